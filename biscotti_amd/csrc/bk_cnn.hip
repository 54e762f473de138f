// bk_cnn.hip -- the forward pass of the reference's one-layer mnist CNN
// (ML/Pytorch/mnist_cnn_model.py: Conv2d(1, c_out, k, 1, pad), ReLU,
// MaxPool2d(1), Linear(c_out oh ow, n_classes)) on resident samples, gfx950
// (DESIGN.md §5y).  One kernel, k_cnn<K>, serves bk_eval's sets and
// bk_roni_cnn_batches' gathered mini-batches; bk.h states its arithmetic.
//
// A logit is ONE fp64 chain over all F = c_out oh ow features in ascending
// order, so it cannot be split across waves: the parallelism is over sample
// tiles.  A workgroup of five waves owns a tile of up to 16 samples of one
// evaluation (the 16 columns of v_mfma_f64_16x16x4_f64):
//
//   staging    the tile's images go once into LDS as zero-padded fp32 planes
//              ((h + 2 pad) x (w + 2 pad), the stride padded to 4 mod 64 words:
//              the 16 samples x 4 features a producer wave reads at once fall
//              into 64 banks), so the tap loop has no bounds test; the conv
//              weights and the biases as doubles of their fp32 values
//   producers  waves 1..4: lane (s = l & 15, q = l >> 4) computes feature
//              k0 + 16 step + 4 (wave - 1) + q of sample s -- the fp64 tap chain
//              of the pre-activation and, beside it, the chain of the taps'
//              magnitudes for the near-tie bound -- into a two-deep LDS ring of
//              64-feature chunks: the activation and its bound operand, fp32
//   consumer   wave 0 walks the ring in feature order: per 4 features one MFMA
//              into the logits (A: the fc weights of 16 class rows, fp32-rounded,
//              prefetched a chunk ahead from L2 into registers; B: the
//              activations) and one into the bound (A's magnitudes, B: the bound
//              operands).  D reg r of lane l is class (l >> 4) + 4 r, sample l & 15
//   one barrier per chunk keeps the two sides a chunk apart; the activations
//   never leave LDS.  Tails (F not a multiple of 4 or 64, rows past C, a tile's
//   missing samples) feed zeros, which leave a chain that started at +0.0 as it is.
//
// Lane s of wave 0 then takes the argmax, the label compare and the near-tie
// test of sample s; thread 0 adds the tile's counts to the launch's counters
// and leaves through round_exit (bk_roni_dev.h): the last workgroup out writes
// the sets' errors into the evaluation entries' mapped block, or the updates'
// scores, and zeroes the counters.  Nobody spins.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bk_internal.h"
#include "bk_roni_dev.h"

namespace bk {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int CNN_NT = 320;                // wave 0 consumes, waves 1..4 produce
constexpr int CNN_KC = 64;                 // features per ring chunk
constexpr int CNN_TS = 16;                 // samples per tile: the MFMA's columns
constexpr int CNN_IMG_BYTES = 96 * 1024;   // the planes' LDS budget
constexpr int CNN_MAX_K = 5, CNN_MAX_CO = 16;

bool cnn_dims(int h, int w, int k, int pad, int co, int C, CnnDims *out) {
    if (k < 1 || k > CNN_MAX_K || pad < 0 || pad >= k || h < 1 || w < 1 || h > 64 || w > 64 ||
        k > h + 2 * pad || k > w + 2 * pad || co < 1 || co > CNN_MAX_CO || C < 2 || C > 16)
        return false;
    CnnDims m = {};
    m.h = h, m.w = w, m.k = k, m.pad = pad, m.co = co, m.C = C;
    m.ph = h + 2 * pad, m.pw = w + 2 * pad;
    m.oh = m.ph - k + 1, m.ow = m.pw - k + 1;
    const int plane = m.ph * m.pw;
    m.ps = plane + ((4 - plane % 64) + 64) % 64;
    const int fit = CNN_IMG_BYTES / (m.ps * (int)sizeof(float));
    m.ts = fit < CNN_TS ? fit : CNN_TS;
    m.F = (int64_t)co * m.oh * m.ow;
    m.d = (int64_t)co * k * k + co + (int64_t)C * m.F + C;
    *out = m;
    return true;
}

static double gamma_u(double n) {
    const double u = 0x1p-24;
    return n * u / (1.0 - n * u);
}

// bk.h's g_F and g_e, in exactly this order of fp64 operations (tests/cnn_ref.py
// repeats them)
void cnn_gammas(const CnnDims &m, double *gF, double *ge) {
    const double g = gamma_u((double)(m.F + 1));
    *gF = g * (1.0 + 0x1p-10);
    *ge = (gamma_u((double)(m.k * m.k + 1)) + 1.001 * 0x1p-24) * (1.0 + g) * (1.0 + 0x1p-20);
}

template <int K>
__global__ __launch_bounds__(CNN_NT) void k_cnn(const CnnLaunch a, double gF, double ge) {
    extern __shared__ __attribute__((aligned(16))) float img[];  // ts planes of ps words
    __shared__ float ring[2][2][CNN_KC][CNN_TS];  // [slot][activation, bound operand]
    __shared__ double cw[CNN_MAX_CO * K * K], cb[CNN_MAX_CO], fb[16];
    __shared__ double eb[CNN_TS][17];
    __shared__ float lt[CNN_TS][17];
    __shared__ int64_t srow[CNN_TS];
    __shared__ int s_last;
    const CnnDims &m = a.m;
    const int tid = threadIdx.x, l = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = m.C, ts = m.ts;
    const int64_t F = m.F;
    const bool batches = a.idx != nullptr;

    // the workgroup's evaluation (a set, or a batch), its tile and its model
    int grp = 0;
    int64_t p0, total;
    EvalSet set = a.desc.s[0];
    const double *dj = nullptr;
    if (batches) {
        const int tpe = cnn_tiles(m, a.nb);
        grp = (int)(blockIdx.x / (unsigned)tpe);
        p0 = (int64_t)(blockIdx.x - (unsigned)grp * (unsigned)tpe) * ts;
        total = a.nb;
        if (grp & 1) dj = a.deltas + (int64_t)(grp >> 1) * a.ld;
    } else {
        int t0 = a.desc.s[0].tile0;  // tile0 ascends with the set
#pragma unroll
        for (int i = 1; i < EVAL_MAX_SETS; ++i)
            if (i < a.desc.nsets && (int)blockIdx.x >= a.desc.s[i].tile0) {
                grp = i;
                t0 = a.desc.s[i].tile0;
                set = a.desc.s[i];
            }
        p0 = (int64_t)((int)blockIdx.x - t0) * ts;
        total = set.nv;
    }
    const float *__restrict__ Xv = (const float *)set.X;
    const int32_t *__restrict__ yv = (const int32_t *)set.y;
    const double *__restrict__ ww = a.ww;
    // entry i of the evaluation's model, as torch.FloatTensor holds it
    auto model = [&](int64_t i) { return (double)(float)(dj ? ww[i] + dj[i] : ww[i]); };
    const int64_t o_cb = (int64_t)m.co * K * K, o_fw = o_cb + m.co, o_fb = o_fw + (int64_t)C * F;

    for (int i = tid; i < m.co * K * K; i += CNN_NT) cw[i] = model(i);
    if (tid < CNN_MAX_CO) cb[tid] = tid < m.co ? model(o_cb + tid) : 0.0;
    if (tid >= 64 && tid < 80) fb[tid - 64] = tid - 64 < C ? model(o_fb + tid - 64) : 0.0;
    if (tid >= 128 && tid < 128 + CNN_TS) {  // the tile's rows; -1: no sample
        const int s = tid - 128;
        int64_t row = -1;
        if (s < ts && p0 + s < total) {
            row = batches ? a.idx[(int64_t)grp * a.nb + p0 + s] : p0 + s;
            if (row < 0 || row >= set.nv) row = 0;  // the host entry has refused it; never out of range
        }
        srow[s] = row;
    }
    __syncthreads();
    {
        const int plane = m.ph * m.pw;
        for (int i = tid; i < ts * plane; i += CNN_NT) {
            const int s = i / plane, r = i - s * plane, yy = r / m.pw, xx = r - yy * m.pw;
            const int64_t row = srow[s];
            const bool in = row >= 0 && yy >= m.pad && yy < m.pad + m.h && xx >= m.pad && xx < m.pad + m.w;
            img[s * m.ps + r] = in ? Xv[row * set.ldv + (int64_t)(yy - m.pad) * m.w + (xx - m.pad)] : 0.0f;
        }
    }
    __syncthreads();

    const int nch = (int)((F + CNN_KC - 1) / CNN_KC);
    const int s16 = l & 15, q4 = l >> 4;
    // producers: chunk ch's activations and bound operands into ring slot `slot`
    auto produce = [&](int ch, int slot) {
        const unsigned plane_o = (unsigned)(m.oh * m.ow);
#pragma unroll 1
        for (int step = 0; step < CNN_KC / 16; ++step) {
            const int fl = 16 * step + 4 * (wave - 1) + q4;
            const int64_t f = (int64_t)ch * CNN_KC + fl;
            float act = 0.0f, bnd = 0.0f;
            if (f < F && s16 < ts) {
                const unsigned fu = (unsigned)f, c = fu / plane_o, r = fu - c * plane_o,
                               y = r / (unsigned)m.ow, x = r - y * (unsigned)m.ow;
                const float *px = img + s16 * m.ps + y * m.pw + x;
                const double *pw = cw + c * (K * K);
                double acc = 0.0, mag = 0.0;
#pragma unroll
                for (int ky = 0; ky < K; ++ky)
#pragma unroll
                    for (int kx = 0; kx < K; ++kx) {
                        const double xv = (double)px[ky * m.pw + kx], wv = pw[ky * K + kx];
                        acc = __builtin_fma(xv, wv, acc);
                        mag = __builtin_fma(__builtin_fabs(xv), __builtin_fabs(wv), mag);
                    }
                const float pre = (float)(acc + cb[c]);
                act = pre < 0.0f ? 0.0f : pre;  // a NaN stays
                const double t = gF * (double)act + ge * (mag + __builtin_fabs(cb[c]));
                bnd = (float)(t * (1.0 + 0x1p-22) + 0x1p-126);  // rounded up
            }
            ring[slot][0][fl][s16] = act;
            ring[slot][1][fl][s16] = bnd;
        }
    };
    // the consumer's A operand: class row s16, features k0 + 4 st + q4, raw
    const bool con = s16 < C;
    const int64_t arow = o_fw + (int64_t)(con ? s16 : 0) * F;
    double wa[CNN_KC / 4], wb[CNN_KC / 4];
    auto load_a = [&](int ch) {
#pragma unroll
        for (int st = 0; st < CNN_KC / 4; ++st) {
            const int64_t f = (int64_t)ch * CNN_KC + 4 * st + q4;
            const int64_t i = arow + (f < F ? f : F - 1);
            wa[st] = ww[i];
            wb[st] = dj ? dj[i] : 0.0;
        }
    };
    d4 acc = d4{0.0, 0.0, 0.0, 0.0}, accb = d4{0.0, 0.0, 0.0, 0.0};
    if (wave > 0)
        produce(0, 0);
    else
        load_a(0);
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
        if (wave > 0) {
            if (ch + 1 < nch) produce(ch + 1, (ch + 1) & 1);
        } else {
            double av[CNN_KC / 4];
#pragma unroll
            for (int st = 0; st < CNN_KC / 4; ++st) {
                const bool on = con && (int64_t)ch * CNN_KC + 4 * st + q4 < F;
                av[st] = on ? (double)(float)(dj ? wa[st] + wb[st] : wa[st]) : 0.0;
            }
            if (ch + 1 < nch) load_a(ch + 1);  // in flight under this chunk's MFMAs
            const int64_t left = F - (int64_t)ch * CNN_KC;
            const int steps = left < CNN_KC ? (int)((left + 3) >> 2) : CNN_KC / 4;
            const int slot = ch & 1;
#pragma unroll
            for (int st = 0; st < CNN_KC / 4; ++st) {
                if (st < steps) {
                    const double b = (double)ring[slot][0][4 * st + q4][s16];
                    const double bb = (double)ring[slot][1][4 * st + q4][s16];
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[st], b, acc, 0, 0, 0);
                    accb = __builtin_amdgcn_mfma_f64_16x16x4f64(__builtin_fabs(av[st]), bb, accb, 0, 0, 0);
                }
            }
        }
        __syncthreads();  // chunk ch is consumed, chunk ch + 1 is in the ring
    }
    if (wave == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = q4 + 4 * r;
            lt[s16][c] = (float)(acc[r] + fb[c]);
            eb[s16][c] = accb[r] + gF * __builtin_fabs(fb[c]);
        }
    }
    __syncthreads();
    bool ok = false, nt = false;
    if (tid < CNN_TS && srow[tid] >= 0) {
        // np.argmax: the first maximum, a NaN wins at its first place
        const float *lg = lt[tid];
        int best = 0;
        float b0 = lg[0];
        for (int c = 1; c < C; ++c) {
            const float v = lg[c];
            if (!(b0 != b0) && (v != v || v > b0)) {
                best = c;
                b0 = v;
            }
        }
        ok = best == yv[srow[tid]];
        double emax = 0.0, l2 = -__builtin_inf();
        bool fin = true;
        for (int c = 0; c < C; ++c) {
            const double v = (double)lg[c], e = eb[tid][c];
            emax = e > emax ? e : emax;
            fin = fin && __builtin_isfinite(v);
            if (c != best && v > l2) l2 = v;
        }
        const double u = 0x1p-24, l1 = (double)lg[best];
        nt = !fin || !(l1 - l2 - u * (__builtin_fabs(l1) + __builtin_fabs(l2)) > eb[tid][best] + emax);
    }
    if (wave == 0) {
        const unsigned int mine[2] = {(unsigned int)__popcll(__ballot(ok)),
                                      (unsigned int)__popcll(__ballot(nt))};
        if (tid == 0) {
            const int64_t g2 = batches ? 2 * a.n : EVAL_MAX_SETS;
            const int slot[2] = {grp, (int)g2 + grp};
            s_last = round_exit(mine, slot, a.cnt, (int)(2 * g2));
        }
    }
    __syncthreads();
    if (!s_last) return;
    // the last workgroup out: the totals, then the counters back to zero
    if (!batches) {
        if (tid != 0) return;
        for (int i = 0; i < a.desc.nsets; ++i) {
            const int64_t nv = a.desc.s[i].nv;
            const unsigned int good = round_load(a.cnt + i), near = round_load(a.cnt + EVAL_MAX_SETS + i);
            a.out->err[i] = 1.0 - (double)good / (double)nv;
            a.out->wrong[i] = nv - (int64_t)good;
            a.out->near[i] = (int32_t)near;
        }
        for (int i = 0; i <= EVAL_EXIT; ++i)
            __hip_atomic_store(a.cnt + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const double dn = (double)a.nb;
    for (int64_t j = tid; j < a.n; j += CNN_NT) {
        unsigned int v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            unsigned int *p = a.cnt + (e >> 1) * 2 * a.n + 2 * j + (e & 1);
            v[e] = round_load(p);
            __hip_atomic_store(p, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const double orig = 1.0 - (double)v[0] / dn, after = 1.0 - (double)v[1] / dn;
        a.scores[j] = after - orig;
        if (a.near) {
            a.near[2 * j] = (int32_t)v[2];
            a.near[2 * j + 1] = (int32_t)v[3];
        }
    }
    if (tid == 0) __hip_atomic_store(a.cnt + 4 * a.n, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int K>
static hipError_t launch_k(const CnnLaunch &a, int64_t tiles, double gF, double ge, hipStream_t st) {
    // per device, so asked on every launch: the planes exceed the default 64 KiB
    const hipError_t e = hipFuncSetAttribute((const void *)k_cnn<K>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, CNN_IMG_BYTES);
    if (e != hipSuccess) return e;
    const size_t lds = (size_t)a.m.ts * a.m.ps * sizeof(float);
    hipLaunchKernelGGL(k_cnn<K>, dim3((unsigned)tiles), dim3(CNN_NT), lds, st, a, gF, ge);
    return hipGetLastError();
}

hipError_t launch_cnn(const CnnLaunch &a, int64_t tiles, hipStream_t st) {
    const CnnDims &m = a.m;
    if (tiles < 1 || tiles > 0x7fffffff || m.ts < 1 || m.ts > CNN_TS || m.k < 1 || m.k > CNN_MAX_K ||
        (size_t)m.ts * m.ps * sizeof(float) > CNN_IMG_BYTES)
        return hipErrorInvalidConfiguration;
    if (a.idx ? a.n < 1 || a.nb < 1 : a.desc.nsets < 1 || a.desc.nsets > EVAL_MAX_SETS)
        return hipErrorInvalidConfiguration;
    double gF, ge;
    cnn_gammas(m, &gF, &ge);
    switch (m.k) {
    case 1: return launch_k<1>(a, tiles, gF, ge, st);
    case 2: return launch_k<2>(a, tiles, gF, ge, st);
    case 3: return launch_k<3>(a, tiles, gF, ge, st);
    case 4: return launch_k<4>(a, tiles, gF, ge, st);
    default: return launch_k<5>(a, tiles, gF, ge, st);
    }
}

}  // namespace bk
