// bk_cnn2.hip -- the forward pass of the reference's two-layer lfw CNN
// (ML/Pytorch/lfw_cnn_model.py: Conv2d(c_in, c1, k, 1, pad), ReLU, MaxPool2d(2),
// Conv2d(c1, c2, k, 1, pad), ReLU, MaxPool2d(2), Linear(c2 ph2 pw2, n_classes))
// on resident samples, gfx950.  One kernel, k_cnn2<K>, serves
// bk_eval's sets and bk_roni_cnn2_batches' gathered mini-batches; bk.h states
// its arithmetic and the near-tie bound.
//
// A workgroup of four waves is ONE sample: the second convolution is the work
// (at lfw 36 x 660 kept outputs over K = 162, twice: the value and its bound),
// and a sample's maps fill the LDS of a CU, so a CU holds one sample.
//
//   staging   the evaluation's conv weights, fp32(ww [+ delta]), into LDS as
//             fp32: conv1's as they lie, conv2's as c2 rows of stride ws = 4 x
//             (an odd number of MFMA steps), zero past K -- the 16 rows x 4 k
//             of an A fragment fall into 64 different banks; a table koff[k] of
//             tap k's offset (ci plane, ky row, kx) in the pooled map
//   conv1     VALU, not MFMA: lane = one pooled position.  It loads the
//             c_in x (k+1) x (k+1) input patch of its 2 x 2 window once from
//             global memory (bounds-tested there: the padding is zeros in
//             registers) and runs, per output channel, the four windows' fp64
//             tap chains and the chains of the taps' magnitudes, a weight read
//             once from LDS (a broadcast) for 8 FMAs.  On the MFMA the same
//             work would fill 18 of 32 rows and 27 of 28 k at lfw: no fewer
//             issue cycles, and the pool would need a pass of its own.  The
//             pooled activation and its bound operand go into LDS as planes
//             zero-padded by `pad` (odd plane stride), so conv2's tap loop has
//             no bounds test; a sample's maps never reach global memory
//   conv2     v_mfma_f64_16x16x4_f64.  An item is (row tile of 16 output
//             channels, column tile of 4 pooled positions x their 4 window
//             elements); the waves take items round-robin.  Per step of 4 taps,
//             k = (ci, ky, kx) ascending: A = the weights (and, for the second
//             accumulator, their magnitudes), B = the pooled map (the bound
//             operands) at koff[k] + the column's window position.  D reg r of
//             lane l is channel (l >> 4) + 4 r, column l & 15, so the 2 x 2 pool
//             is a maximum over the lane quad l ^ 1, l ^ 2.  The quad's first
//             lane writes the pooled activation and its fc bound operand into
//             the tile's scratch, [feature][16 samples]: the fc MFMA's B operand
//   fc        the 16 samples of a tile count themselves out on the tile's
//             counter (grad_last_out: release, counter, acquire); the one that
//             leaves last runs the tile's chains over all F features, wave 0
//             the logits' and wave 1 the bound's, one dependent MFMA per 4
//             features, the next 64 features' operands in flight in registers.
//             Nobody waits for anybody.
//
// Lane s of wave 0 then takes argmax, label compare and near-tie test of sample
// s; every workgroup leaves through round_exit (bk_roni_dev.h) and the launch's
// last one out writes the sets' errors or the updates' scores and zeroes the
// counters, as k_cnn does.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bk_grad_dev.h"
#include "bk_internal.h"
#include "bk_roni_dev.h"

namespace bk {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int C2_NT = 256;
constexpr int C2_LDS_BYTES = 150 * 1024;  // the dynamic LDS budget (the CU has 160 KiB)
constexpr int C2_FC = 16;                 // fc steps in flight: 64 features

bool cnn2_dims(int c_in, int h, int w, int k, int pad, int c1, int c2, int C, Cnn2Dims *out) {
    if (c_in < 1 || c_in > 3 || h < 2 || w < 2 || h > 64 || w > 64 || k < 1 || k > 3 || pad < 0 ||
        pad >= k || c1 < 1 || c1 > 32 || c2 < 1 || c2 > 48 || C < 2 || C > 16)
        return false;
    Cnn2Dims m = {};
    m.c_in = c_in, m.h = h, m.w = w, m.k = k, m.pad = pad, m.c1 = c1, m.c2 = c2, m.C = C;
    m.ph1 = (h + 2 * pad - k + 1) / 2, m.pw1 = (w + 2 * pad - k + 1) / 2;
    if (m.ph1 < 1 || m.pw1 < 1) return false;
    m.P1h = m.ph1 + 2 * pad, m.P1w = m.pw1 + 2 * pad;
    m.ps1 = (m.P1h * m.P1w) | 1;
    m.ph2 = (m.P1h - k + 1) / 2, m.pw2 = (m.P1w - k + 1) / 2;
    if (m.ph2 < 1 || m.pw2 < 1) return false;
    m.np2 = m.ph2 * m.pw2;
    m.T1 = c_in * k * k, m.T2 = c1 * k * k;
    m.st2 = (m.T2 + 3) / 4;
    m.ws = 4 * (m.st2 | 1);
    m.lds = 4 * (2 * c1 * m.ps1 + c2 * m.ws + c1 * m.T1 + c1 + c2 + 4 * m.st2);
    if (m.lds > C2_LDS_BYTES) return false;
    m.F = (int64_t)c2 * m.np2;
    m.F4 = (m.F + 3) / 4 * 4;
    m.d = (int64_t)c1 * m.T1 + c1 + (int64_t)c2 * m.T2 + c2 + (int64_t)C * m.F + C;
    *out = m;
    return true;
}

static double gamma_u(double n) {
    const double u = 0x1p-24;
    return n * u / (1.0 - n * u);
}

// bk.h's factors, in exactly this order of fp64 operations
Cnn2Gammas cnn2_gammas(const Cnn2Dims &m) {
    const double u = 0x1p-24, s = 1.0 + 0x1p-20;
    const double c1 = gamma_u((double)(m.T1 + 1)), c2 = gamma_u((double)(m.T2 + 1)),
                 cF = gamma_u((double)(m.F + 1));
    Cnn2Gammas g;
    g.g1 = (c1 + 1.001 * u) * s;
    g.g2 = (c2 + 1.001 * u) * s;
    g.h2 = (1.0 + c2) * s;
    g.gF = cF * (1.0 + 0x1p-10);
    g.hF = (1.0 + cF) * s;
    return g;
}

// bk.h's fp32_up: not below t
__device__ __forceinline__ float up32(double t) { return (float)(t * (1.0 + 0x1p-22) + 0x1p-126); }
// the pool's maximum: a NaN in the window stays
__device__ __forceinline__ float pmax(float a, float b) { return a != a ? a : (b != b || b > a) ? b : a; }

template <int K>
__global__ __launch_bounds__(C2_NT) void k_cnn2(const Cnn2Launch a, const Cnn2Gammas g) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double fb[16];
    __shared__ double eb[CNN2_TS][17];
    __shared__ float lt[CNN2_TS][17];
    __shared__ int64_t srow[CNN2_TS];
    __shared__ unsigned int s_cons;
    __shared__ int s_last;
    const Cnn2Dims &m = a.m;
    const int tid = threadIdx.x, l = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = m.C, c1 = m.c1, c2 = m.c2, T1 = m.T1, T2 = m.T2, ps1 = m.ps1, P1w = m.P1w;
    const int64_t F = m.F;
    const bool batches = a.idx != nullptr;
    float *const A1 = lds, *const Q1 = A1 + c1 * ps1, *const W2s = Q1 + c1 * ps1,
                 *const W1s = W2s + c2 * m.ws, *const B1 = W1s + c1 * T1, *const B2 = B1 + c1;
    int *const koff = (int *)(B2 + c2);

    // the workgroup's evaluation (a set, or a batch), its sample, its tile and its model
    int grp = 0;
    int64_t p, total, tile;
    EvalSet set = a.desc.s[0];
    const double *dj = nullptr;
    if (batches) {
        grp = (int)((int64_t)blockIdx.x / a.nb);
        p = (int64_t)blockIdx.x - (int64_t)grp * a.nb;
        total = a.nb;
        tile = (int64_t)grp * ((a.nb + CNN2_TS - 1) / CNN2_TS);
        if (grp & 1) dj = a.deltas + (int64_t)(grp >> 1) * a.ld;
    } else {
        tile = 0;
#pragma unroll
        for (int i = 1; i < EVAL_MAX_SETS; ++i)
            if (i < a.desc.nsets && (int)blockIdx.x >= a.desc.s[i].tile0) {  // tile0 ascends with the set
                grp = i;
                set = a.desc.s[i];
            }
#pragma unroll
        for (int i = 0; i < EVAL_MAX_SETS - 1; ++i)
            if (i < grp) tile += (a.desc.s[i].nv + CNN2_TS - 1) / CNN2_TS;
        p = (int64_t)((int)blockIdx.x - set.tile0);
        total = set.nv;
    }
    const int64_t p0 = p & ~(int64_t)(CNN2_TS - 1);  // the tile's first sample
    tile += p / CNN2_TS;
    const int col = (int)(p - p0);
    const unsigned int pop = (unsigned int)(total - p0 < CNN2_TS ? total - p0 : CNN2_TS);
    const float *__restrict__ Xv = (const float *)set.X;
    const int32_t *__restrict__ yv = (const int32_t *)set.y;
    const double *__restrict__ ww = a.ww;
    auto sample = [&](int64_t q) {  // sample q of the evaluation: its row in the set
        int64_t row = batches ? a.idx[(int64_t)grp * a.nb + q] : q;
        if (row < 0 || row >= set.nv) row = 0;  // the host entry has refused it; never out of range
        return row;
    };
    // entry i of the evaluation's model, as torch.FloatTensor holds it
    auto model = [&](int64_t i) { return (float)(dj ? ww[i] + dj[i] : ww[i]); };
    const int64_t o_b1 = (int64_t)c1 * T1, o_w2 = o_b1 + c1, o_b2 = o_w2 + (int64_t)c2 * T2,
                  o_fw = o_b2 + c2, o_fb = o_fw + (int64_t)C * F;

    for (int i = tid; i < c1 * T1; i += C2_NT) W1s[i] = model(i);
    for (int i = tid; i < c1; i += C2_NT) B1[i] = model(o_b1 + i);
    for (int i = tid; i < c2; i += C2_NT) B2[i] = model(o_b2 + i);
    for (int i = tid; i < c2 * m.ws; i += C2_NT) {
        const int r = i / m.ws, k = i - r * m.ws;
        W2s[i] = k < T2 ? model(o_w2 + (int64_t)r * T2 + k) : 0.0f;
    }
    for (int k = tid; k < 4 * m.st2; k += C2_NT) {
        const int ci = k / (K * K), t = k - ci * (K * K), ky = t / K, kx = t - ky * K;
        koff[k] = k < T2 ? ci * ps1 + ky * P1w + kx : 0;
    }
    for (int i = tid; i < 2 * c1 * ps1; i += C2_NT) A1[i] = 0.0f;  // A1 and Q1: the borders stay zero
    __syncthreads();

    // ---- conv1, ReLU, pool: lane = pooled position, all channels
    {
        const float *__restrict__ img = Xv + sample(p) * set.ldv;
        const int hw = m.h * m.w;
        for (int pos = tid; pos < m.ph1 * m.pw1; pos += C2_NT) {
            const int py = pos / m.pw1, px = pos - py * m.pw1;
            double x[3][K + 1][K + 1];
#pragma unroll
            for (int ci = 0; ci < 3; ++ci)
#pragma unroll
                for (int r = 0; r <= K; ++r)
#pragma unroll
                    for (int s = 0; s <= K; ++s) {
                        const int iy = 2 * py - m.pad + r, ix = 2 * px - m.pad + s;
                        const bool in = ci < m.c_in && iy >= 0 && iy < m.h && ix >= 0 && ix < m.w;
                        x[ci][r][s] = in ? (double)img[ci * hw + iy * m.w + ix] : 0.0;
                    }
            const int o = (py + m.pad) * P1w + px + m.pad;
#pragma unroll 1
            for (int c = 0; c < c1; ++c) {
                const float *pw = W1s + c * T1;
                double acc[4] = {0.0, 0.0, 0.0, 0.0}, mag[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int ci = 0; ci < 3; ++ci)
                    if (ci < m.c_in) {
#pragma unroll
                        for (int ky = 0; ky < K; ++ky)
#pragma unroll
                            for (int kx = 0; kx < K; ++kx) {
                                const double wv = (double)pw[(ci * K + ky) * K + kx], aw = __builtin_fabs(wv);
#pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    const double xv = x[ci][ky + (e >> 1)][kx + (e & 1)];
                                    acc[e] = __builtin_fma(xv, wv, acc[e]);
                                    mag[e] = __builtin_fma(__builtin_fabs(xv), aw, mag[e]);
                                }
                            }
                    }
                const double bias = (double)B1[c];
                float av = 0.0f, tv = 0.0f;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float pre = (float)(acc[e] + bias);
                    const float act = pre < 0.0f ? 0.0f : pre;  // a NaN stays
                    const float t = up32(g.g1 * (mag[e] + __builtin_fabs(bias)));
                    av = e ? pmax(av, act) : act;
                    tv = e ? pmax(tv, t) : t;
                }
                A1[c * ps1 + o] = av;
                Q1[c * ps1 + o] = up32(g.g2 * (double)av + g.h2 * (double)tv);
            }
        }
    }
    __syncthreads();

    // ---- conv2 on the MFMA, ReLU, pool, into the tile's scratch
    const int s16 = l & 15, q4 = l >> 4;
    float *const sa = a.scratch + (size_t)tile * cnn2_tile_floats(m);
    float *const sb = sa + (size_t)m.F4 * CNN2_TS;
    {
        const int nrt = (c2 + 15) >> 4, nct = (m.np2 + 3) >> 2;
#pragma unroll 1
        for (int item = wave; item < nrt * nct; item += C2_NT / 64) {
            const int ct = item / nrt, rt = item - ct * nrt;
            const int pp = 4 * ct + (s16 >> 2), ppc = pp < m.np2 ? pp : 0;
            const int py = ppc / m.pw2, px = ppc - py * m.pw2;
            const int pbase = (2 * py + ((s16 >> 1) & 1)) * P1w + 2 * px + (s16 & 1);
            const int arow = 16 * rt + s16;
            const bool aon = arow < c2;
            const float *wrow = W2s + (aon ? arow : 0) * m.ws;
            d4 acc = d4{0.0, 0.0, 0.0, 0.0}, accb = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
            for (int st = 0; st < m.st2; ++st) {
                const int k = 4 * st + q4;
                const int o = koff[k] + pbase;
                const bool kin = k < T2;
                const double wv = aon ? (double)wrow[k] : 0.0;  // zero past T2
                const double b = kin ? (double)A1[o] : 0.0, bb = kin ? (double)Q1[o] : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wv, b, acc, 0, 0, 0);
                accb = __builtin_amdgcn_mfma_f64_16x16x4f64(__builtin_fabs(wv), bb, accb, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = 16 * rt + q4 + 4 * r;
                const double bias = (double)B2[c < c2 ? c : 0];
                const float pre = (float)(acc[r] + bias);
                float act = pre < 0.0f ? 0.0f : pre;  // a NaN stays
                float t = up32(accb[r] + g.g2 * __builtin_fabs(bias));
                act = pmax(act, __shfl_xor(act, 1));
                t = pmax(t, __shfl_xor(t, 1));
                act = pmax(act, __shfl_xor(act, 2));
                t = pmax(t, __shfl_xor(t, 2));
                if ((s16 & 3) == 0 && c < c2 && pp < m.np2) {
                    const size_t e = ((size_t)c * m.np2 + pp) * CNN2_TS + col;
                    sa[e] = act;
                    sb[e] = up32(g.gF * (double)act + g.hF * (double)t);
                }
            }
        }
    }
    // the tile's last sample out goes on as its consumer and sees the others' stores
    const bool consumer = grad_last_out(a.tcnt + tile, pop, &s_cons);

    unsigned int mine[2] = {0u, 0u};
    if (consumer) {
        if (tid < 16) fb[tid] = tid < C ? (double)model(o_fb + tid) : 0.0;
        if (tid >= 64 && tid < 64 + CNN2_TS) {  // the tile's rows; -1: no sample
            const int s = tid - 64;
            srow[s] = s < (int)pop ? sample(p0 + s) : -1;
        }
        __syncthreads();
        if (wave < 2) {
            const bool con = s16 < C;
            const int64_t arow = o_fw + (int64_t)(con ? s16 : 0) * F;
            const float *sB = wave ? sb : sa;
            const int nsteps = (int)(m.F4 >> 2), nch = (nsteps + C2_FC - 1) / C2_FC;
            double wa[C2_FC], wd[C2_FC];
            float bv[C2_FC];
            auto load = [&](int ch) {
#pragma unroll
                for (int st = 0; st < C2_FC; ++st) {
                    const int64_t f = (int64_t)ch * (4 * C2_FC) + 4 * st + q4, fc = f < F ? f : F - 1;
                    wa[st] = ww[arow + fc];
                    wd[st] = dj ? dj[arow + fc] : 0.0;
                    bv[st] = sB[(size_t)fc * CNN2_TS + s16];
                }
            };
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};  // wave 0: the logits; wave 1: the bound
            load(0);
#pragma unroll 1
            for (int ch = 0; ch < nch; ++ch) {
                double av[C2_FC], b[C2_FC];
#pragma unroll
                for (int st = 0; st < C2_FC; ++st) {
                    const bool on = (int64_t)ch * (4 * C2_FC) + 4 * st + q4 < F;
                    const double w = on && con ? (double)(float)(dj ? wa[st] + wd[st] : wa[st]) : 0.0;
                    av[st] = wave ? __builtin_fabs(w) : w;
                    b[st] = on ? (double)bv[st] : 0.0;
                }
                if (ch + 1 < nch) load(ch + 1);  // in flight under this chunk's MFMAs
                const int steps = nsteps - ch * C2_FC < C2_FC ? nsteps - ch * C2_FC : C2_FC;
#pragma unroll
                for (int st = 0; st < C2_FC; ++st)
                    if (st < steps) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[st], b[st], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = q4 + 4 * r;
                if (wave == 0)
                    lt[s16][c] = (float)(acc[r] + fb[c]);
                else
                    eb[s16][c] = acc[r] + g.gF * __builtin_fabs(fb[c]);
            }
        }
        __syncthreads();
        bool ok = false, nt = false;
        if (tid < CNN2_TS && srow[tid] >= 0) {
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
            mine[0] = (unsigned int)__popcll(__ballot(ok));
            mine[1] = (unsigned int)__popcll(__ballot(nt));
        }
    }
    if (tid == 0) {
        const int64_t g2 = batches ? 2 * a.n : EVAL_MAX_SETS;
        const int slot[2] = {grp, (int)g2 + grp};
        s_last = round_exit(mine, slot, a.cnt, (int)(2 * g2));
    }
    __syncthreads();
    if (!s_last) return;
    // the launch's last workgroup out: the totals, then the counters back to zero
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
    for (int64_t j = tid; j < a.n; j += C2_NT) {
        unsigned int v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            unsigned int *q = a.cnt + (e >> 1) * 2 * a.n + 2 * j + (e & 1);
            v[e] = round_load(q);
            __hip_atomic_store(q, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
static hipError_t launch_k(const Cnn2Launch &a, int64_t samples, hipStream_t st) {
    // per device, so asked on every launch: the maps exceed the default 64 KiB
    const hipError_t e = hipFuncSetAttribute((const void *)k_cnn2<K>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, C2_LDS_BYTES);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cnn2<K>, dim3((unsigned)samples), dim3(C2_NT), (size_t)a.m.lds, st, a,
                       cnn2_gammas(a.m));
    return hipGetLastError();
}

hipError_t launch_cnn2(const Cnn2Launch &a, int64_t samples, hipStream_t st) {
    const Cnn2Dims &m = a.m;
    if (samples < 1 || samples > 0x7fffffff || m.k < 1 || m.k > 3 || m.c_in < 1 || m.c_in > 3 ||
        m.lds < 1 || m.lds > C2_LDS_BYTES || !a.scratch || !a.tcnt || !a.cnt)
        return hipErrorInvalidConfiguration;
    if (a.idx ? a.n < 1 || a.nb < 1 || samples != 2 * a.n * a.nb
              : a.desc.nsets < 1 || a.desc.nsets > EVAL_MAX_SETS)
        return hipErrorInvalidConfiguration;
    switch (m.k) {
    case 1: return launch_k<1>(a, samples, st);
    case 2: return launch_k<2>(a, samples, st);
    default: return launch_k<3>(a, samples, st);
    }
}

}  // namespace bk
