// bk_cnnc.hip -- the forward pass of the reference's one-layer cifar CNN
// (ML/Pytorch/cifar_cnn_model.py: Conv2d(c_in, c_out, k, 1, pad), ReLU,
// MaxPool2d(1), Linear(c_out oh ow, n_classes)) on resident samples, gfx950
// (DESIGN.md §5ae).  One kernel, k_cnnc<K>, serves bk_eval's sets and
// bk_roni_cnnc_batches' gathered mini-batches; bk.h states its arithmetic.
//
// A logit is ONE fp64 chain over all F = c_out oh ow features in ascending
// order, so the parallelism is over tiles of 16 samples (the 16 columns of
// v_mfma_f64_16x16x4_f64), as in k_cnn (bk_cnn.hip).  What is new is how the
// images reach the producers: a tile is ALWAYS 16 samples, because the
// workgroup never holds whole planes.
//
//   the row stream   Features run (channel, y, x), and output row y of any
//              channel reads padded input rows y .. y + k - 1 of the c_in
//              planes.  Number the padded rows of channel c as v = c ph + y:
//              since oh + k - 1 = ph, the walk over all channels reads the
//              "virtual" rows v = 0 .. c_out ph - 1 through a window that only
//              moves forward.  Virtual row v is padded row v mod ph of every
//              plane (zero if it lies in the padding), and lives in ring slot
//              v mod D.
//   the band ring    [plane][slot][x][sample] fp32 in LDS: word (x, s) of a row
//              is x 16 + s, so the 16 samples x 4 consecutive features a
//              producer wave reads at once are 64 consecutive words -- 64
//              banks, whatever x.  The row stride W is pw rounded up to ow mod
//              4, so that the 4 features stay in distinct banks across a row's
//              end (except where the ring wraps, a two-way conflict once in D
//              rows).  D is the largest span of rows two consecutive chunks
//              need (cnnc_dims): while the producers read chunk ch + 1's rows,
//              the stagers write chunk ch + 2's new rows into other slots, so
//              the chunk barrier orders the ring too.
//   chunks     64 features, CUT at a channel's end (the last chunk of a channel
//              is short; its missing features feed zeros, which leave a chain
//              that started at +0.0 as it is).  So a chunk's conv weights are
//              wave-uniform and a lane keeps one tap row of them in registers
//              for its four features: the tap loop runs (ci, ky) outside, the
//              lane's 4 features inside, kx innermost -- every feature's chain
//              still runs (ci, ky, kx) ascending.
//   stagers    waves 5..7 load the rows chunk ch + 2 adds, one (row, plane) per
//              wave and turn: lane (s = l & 15, q = l >> 4) loads 16 bytes of
//              sample s's row (4 x-quads a pass, all passes of a row in flight
//              together) and writes them as four words, rotated by q so that a
//              store's 64 lanes hit 64 banks.  A row in the padding is written
//              as zeros without a load; the x-padding is zeroed once.
//   producers  waves 1..4: lane (s, q) computes features 16 step + 4 (wave - 1)
//              + q of the chunk for sample s -- the pre-activation's fp64 chain
//              and the magnitudes' beside it -- into the two-deep activation
//              ring, as in k_cnn.
//   consumer   wave 0: k_cnn's, with the chunk's features at c Fc + 64 j + ..
//   one barrier per chunk; nobody spins; the activations never leave LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bk_internal.h"
#include "bk_roni_dev.h"

namespace bk {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int CC_NT = 512;                  // wave 0 consumes, 1..4 produce, 5..7 stage
constexpr int CC_KC = 64;                   // features per ring chunk
constexpr int CC_TS = CNNC_TS;              // samples per tile: the MFMA's columns
constexpr int CC_STAGERS = 3, CC_MAX_Q = 4; // staging waves; passes of 4 x-quads a row (w <= 64)
constexpr int CC_MAX_K = 5, CC_MAX_CO = 32;
constexpr int CC_DYN_MAX = 136 * 1024;      // dynamic LDS: 160 KiB less the static arrays below

// the first and the last virtual row chunk ch reads (a chunk past the end reads the last one's)
__host__ __device__ inline int cnnc_lo(const CnncDims &m, int ch) {
    const int c = ch / m.nchc, j = ch - c * m.nchc;
    return c * m.ph + (j * CC_KC) / m.ow;
}
__host__ __device__ inline int cnnc_hi(const CnncDims &m, int ch) {
    if (ch >= m.co * m.nchc) ch = m.co * m.nchc - 1;
    const int c = ch / m.nchc, j = ch - c * m.nchc;
    int fl = j * CC_KC + CC_KC - 1;
    if (fl > m.Fc - 1) fl = m.Fc - 1;
    return c * m.ph + fl / m.ow + m.k - 1;
}

bool cnnc_dims(int c_in, int h, int w, int k, int pad, int co, int C, CnncDims *out, bool *lds_ok) {
    if (c_in < 1 || c_in > 4 || k < 1 || k > CC_MAX_K || pad < 0 || pad > k || h < 1 || w < 1 || h > 64 ||
        w > 64 || k > h + 2 * pad || k > w + 2 * pad || co < 1 || co > CC_MAX_CO || C < 2 || C > 16)
        return false;
    CnncDims m = {};
    m.c_in = c_in, m.h = h, m.w = w, m.k = k, m.pad = pad, m.co = co, m.C = C;
    m.ph = h + 2 * pad, m.pw = w + 2 * pad;
    m.oh = m.ph - k + 1, m.ow = m.pw - k + 1;
    m.T = c_in * k * k;
    m.Fc = m.oh * m.ow;
    m.nchc = (m.Fc + CC_KC - 1) / CC_KC;
    m.W = m.pw + (4 - (k - 1) % 4) % 4;  // = ow mod 4
    m.D = 1;
    for (int ch = 0; ch < co * m.nchc; ++ch) {
        const int span = cnnc_hi(m, ch + 1) - cnnc_lo(m, ch) + 1;
        if (span > m.D) m.D = span;
    }
    const int64_t lds = (int64_t)((co * m.T + 1) & ~1) * 8 + (int64_t)c_in * m.D * m.W * CC_TS * 4;
    m.lds = (int)lds;
    m.F = (int64_t)co * m.Fc;
    m.d = (int64_t)co * m.T + co + (int64_t)C * m.F + C;
    *out = m;
    *lds_ok = lds <= CC_DYN_MAX;
    return true;
}

static double gamma_u(double n) {
    const double u = 0x1p-24;
    return n * u / (1.0 - n * u);
}

// bk.h's g_F and g_e, in exactly this order of fp64 operations (tests/cnnc_ref.py
// repeats them)
void cnnc_gammas(const CnncDims &m, double *gF, double *ge) {
    const double g = gamma_u((double)(m.F + 1));
    *gF = g * (1.0 + 0x1p-10);
    *ge = (gamma_u((double)(m.T + 1)) + 1.001 * 0x1p-24) * (1.0 + g) * (1.0 + 0x1p-20);
}

template <int K>
__global__ __launch_bounds__(CC_NT) void k_cnnc(const CnncLaunch a, double gF, double ge) {
    extern __shared__ __attribute__((aligned(16))) double dyn[];  // cw, then the band ring
    __shared__ float ring[2][2][CC_KC][CC_TS];  // [slot][activation, bound operand]
    __shared__ double cb[CC_MAX_CO], fb[16];
    __shared__ double eb[CC_TS][17];
    __shared__ float lt[CC_TS][17];
    __shared__ int64_t srow[CC_TS];
    __shared__ int s_last;
    const CnncDims &m = a.m;
    const int tid = threadIdx.x, l = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = m.C, D = m.D, W = m.W, Fc = m.Fc, T = m.T;
    const int64_t F = m.F;
    const bool batches = a.idx != nullptr;
    double *cw = dyn;
    float *band = (float *)(dyn + ((m.co * T + 1) & ~1));  // 16-byte aligned
    const int band_words = m.c_in * D * W * CC_TS;  // a multiple of 4

    // the workgroup's evaluation (a set, or a batch), its tile and its model
    int grp = 0;
    int64_t p0, total;
    EvalSet set = a.desc.s[0];
    const double *dj = nullptr;
    if (batches) {
        const int tpe = cnnc_tiles(a.nb);
        grp = (int)(blockIdx.x / (unsigned)tpe);
        p0 = (int64_t)(blockIdx.x - (unsigned)grp * (unsigned)tpe) * CC_TS;
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
        p0 = (int64_t)((int)blockIdx.x - t0) * CC_TS;
        total = set.nv;
    }
    const float *__restrict__ Xv = (const float *)set.X;
    const int32_t *__restrict__ yv = (const int32_t *)set.y;
    const double *__restrict__ ww = a.ww;
    // entry i of the evaluation's model, as torch.FloatTensor holds it
    auto model = [&](int64_t i) { return (double)(float)(dj ? ww[i] + dj[i] : ww[i]); };
    const int64_t o_cb = (int64_t)m.co * T, o_fw = o_cb + m.co, o_fb = o_fw + (int64_t)C * F;

    for (int i = tid; i < m.co * T; i += CC_NT) cw[i] = model(i);
    if (tid < CC_MAX_CO) cb[tid] = tid < m.co ? model(o_cb + tid) : 0.0;
    if (tid >= 64 && tid < 80) fb[tid - 64] = tid - 64 < C ? model(o_fb + tid - 64) : 0.0;
    if (tid >= 128 && tid < 128 + CC_TS) {  // the tile's rows; -1: no sample
        const int s = tid - 128;
        int64_t row = -1;
        if (p0 + s < total) {
            row = batches ? a.idx[(int64_t)grp * a.nb + p0 + s] : p0 + s;
            if (row < 0 || row >= set.nv) row = 0;  // the host entry has refused it; never out of range
        }
        srow[s] = row;
    }
    for (int i = tid; i < band_words / 4; i += CC_NT) ((f4 *)band)[i] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    __syncthreads();

    const int s16 = l & 15, q4 = l >> 4;
    // staging: virtual rows [va, vb) of every plane into their slots, wave `turn` of `of`
    const bool vec = ((m.w | set.ldv) & 3) == 0;
    const int nq = (m.w + 3) >> 2;
    const int64_t my_row = srow[s16];
    const float *my_x = Xv + (my_row < 0 ? 0 : my_row) * set.ldv;
    auto stage = [&](int va, int vb, int turn, int of) {
        const int rows = (vb - va) * m.c_in;
#pragma unroll 1
        for (int r = turn; r < rows; r += of) {
            const int dv = r / m.c_in, ci = r - dv * m.c_in, v = va + dv;
            const int yy = v % m.ph - m.pad;
            const bool data = yy >= 0 && yy < m.h && my_row >= 0;
            const float *src = my_x + ((int64_t)ci * m.h + yy) * m.w;
            float *dst = band + ((ci * D + v % D) * W + m.pad) * CC_TS + s16;
            f4 val[CC_MAX_Q];
#pragma unroll
            for (int p = 0; p < CC_MAX_Q; ++p) {
                const int x0 = 4 * (4 * p + q4);
                val[p] = f4{0.0f, 0.0f, 0.0f, 0.0f};
                if (data && 4 * p + q4 < nq) {
                    if (vec)
                        val[p] = *(const f4 *)(src + x0);
                    else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (x0 + e < m.w) val[p][e] = src[x0 + e];
                    }
                }
            }
#pragma unroll
            for (int p = 0; p < CC_MAX_Q; ++p) {
                const int x0 = 4 * (4 * p + q4);
                if (4 * p + q4 < nq) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int e = (j + q4) & 3;  // lane quarter q4 starts at its own element
                        const float t = e == 0 ? val[p][0] : e == 1 ? val[p][1] : e == 2 ? val[p][2] : val[p][3];
                        if (x0 + e < m.w) dst[(x0 + e) * CC_TS] = t;
                    }
                }
            }
        }
    };
    stage(0, cnnc_hi(m, 0) + 1, wave, CC_NT / 64);
    __syncthreads();

    const int nch = m.co * m.nchc;
    // producers: chunk ch's activations and bound operands into ring slot `slot`
    auto produce = [&](int ch, int slot) {
        const int c = ch / m.nchc, j = ch - c * m.nchc;
        const double *pw = cw + c * T;
        int sl[4], xo[4];
        bool on[4];
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const int fl = j * CC_KC + 16 * st + 4 * (wave - 1) + q4;
            on[st] = fl < Fc;
            const unsigned fc = (unsigned)(on[st] ? fl : Fc - 1), y = fc / (unsigned)m.ow;
            xo[st] = (int)(fc - y * (unsigned)m.ow) * CC_TS + s16;
            sl[st] = (c * m.ph + (int)y) % D;
        }
        double acc[4] = {0.0, 0.0, 0.0, 0.0}, mag[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
        for (int ci = 0; ci < m.c_in; ++ci) {
#pragma unroll
            for (int ky = 0; ky < K; ++ky) {
                double wv[K];
#pragma unroll
                for (int kx = 0; kx < K; ++kx) wv[kx] = pw[(ci * K + ky) * K + kx];
#pragma unroll
                for (int st = 0; st < 4; ++st) {
                    int r = sl[st] + ky;
                    r = r >= D ? r - D : r;
                    const float *px = band + (ci * D + r) * W * CC_TS + xo[st];
#pragma unroll
                    for (int kx = 0; kx < K; ++kx) {
                        const double xv = (double)px[kx * CC_TS];
                        acc[st] = __builtin_fma(xv, wv[kx], acc[st]);
                        mag[st] = __builtin_fma(__builtin_fabs(xv), __builtin_fabs(wv[kx]), mag[st]);
                    }
                }
            }
        }
        const double bias = cb[c];
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const int fl = 16 * st + 4 * (wave - 1) + q4;
            const float pre = (float)(acc[st] + bias);
            float act = pre < 0.0f ? 0.0f : pre;  // a NaN stays
            const double t = gF * (double)act + ge * (mag[st] + __builtin_fabs(bias));
            float bnd = (float)(t * (1.0 + 0x1p-22) + 0x1p-126);  // rounded up
            if (!on[st]) act = bnd = 0.0f;
            ring[slot][0][fl][s16] = act;
            ring[slot][1][fl][s16] = bnd;
        }
    };
    // the consumer's A operand: class row s16, features c Fc + 64 j + 4 st + q4, raw
    const bool con = s16 < C;
    const int64_t arow = o_fw + (int64_t)(con ? s16 : 0) * F;
    double wa[CC_KC / 4], wb[CC_KC / 4];
    auto load_a = [&](int ch) {
        const int c = ch / m.nchc, j = ch - c * m.nchc;
#pragma unroll
        for (int st = 0; st < CC_KC / 4; ++st) {
            const int g = j * CC_KC + 4 * st + q4;
            const int64_t i = arow + (int64_t)c * Fc + (g < Fc ? g : Fc - 1);
            wa[st] = ww[i];
            wb[st] = dj ? dj[i] : 0.0;
        }
    };
    d4 acc = d4{0.0, 0.0, 0.0, 0.0}, accb = d4{0.0, 0.0, 0.0, 0.0};
    if (wave == 0)
        load_a(0);
    else if (wave <= 4)
        produce(0, 0);
    else
        stage(cnnc_hi(m, 0) + 1, cnnc_hi(m, 1) + 1, wave - 5, CC_STAGERS);
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
        if (wave > 4) {
            stage(cnnc_hi(m, ch + 1) + 1, cnnc_hi(m, ch + 2) + 1, wave - 5, CC_STAGERS);
        } else if (wave > 0) {
            if (ch + 1 < nch) produce(ch + 1, (ch + 1) & 1);
        } else {
            const int j = ch % m.nchc;
            double av[CC_KC / 4];
#pragma unroll
            for (int st = 0; st < CC_KC / 4; ++st) {
                const bool on = con && j * CC_KC + 4 * st + q4 < Fc;
                av[st] = on ? (double)(float)(dj ? wa[st] + wb[st] : wa[st]) : 0.0;
            }
            if (ch + 1 < nch) load_a(ch + 1);  // in flight under this chunk's MFMAs
            const int left = Fc - j * CC_KC;
            const int steps = left < CC_KC ? (left + 3) >> 2 : CC_KC / 4;
            const int slot = ch & 1;
#pragma unroll
            for (int st = 0; st < CC_KC / 4; ++st) {
                if (st < steps) {
                    const double b = (double)ring[slot][0][4 * st + q4][s16];
                    const double bb = (double)ring[slot][1][4 * st + q4][s16];
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[st], b, acc, 0, 0, 0);
                    accb = __builtin_amdgcn_mfma_f64_16x16x4f64(__builtin_fabs(av[st]), bb, accb, 0, 0, 0);
                }
            }
        }
        __syncthreads();  // chunk ch is consumed, chunk ch + 1 is in the ring, chunk ch + 2's rows in the band
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
    if (tid < CC_TS && srow[tid] >= 0) {
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
    for (int64_t j = tid; j < a.n; j += CC_NT) {
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
static hipError_t launch_k(const CnncLaunch &a, int64_t tiles, double gF, double ge, hipStream_t st) {
    // per device, so asked on every launch: the ring may exceed the default 64 KiB
    const hipError_t e = hipFuncSetAttribute((const void *)k_cnnc<K>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, CC_DYN_MAX);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cnnc<K>, dim3((unsigned)tiles), dim3(CC_NT), (size_t)a.m.lds, st, a, gF, ge);
    return hipGetLastError();
}

hipError_t launch_cnnc(const CnncLaunch &a, int64_t tiles, hipStream_t st) {
    const CnncDims &m = a.m;
    if (tiles < 1 || tiles > 0x7fffffff || m.k < 1 || m.k > CC_MAX_K || m.w > 16 * CC_MAX_Q || m.D < 1 ||
        m.lds < 1 || m.lds > CC_DYN_MAX)
        return hipErrorInvalidConfiguration;
    if (a.idx ? a.n < 1 || a.nb < 1 : a.desc.nsets < 1 || a.desc.nsets > EVAL_MAX_SETS)
        return hipErrorInvalidConfiguration;
    double gF, ge;
    cnnc_gammas(m, &gF, &ge);
    switch (m.k) {
    case 1: return launch_k<1>(a, tiles, gF, ge, st);
    case 2: return launch_k<2>(a, tiles, gF, ge, st);
    case 3: return launch_k<3>(a, tiles, gF, ge, st);
    case 4: return launch_k<4>(a, tiles, gF, ge, st);
    default: return launch_k<5>(a, tiles, gF, ge, st);
    }
}

}  // namespace bk
