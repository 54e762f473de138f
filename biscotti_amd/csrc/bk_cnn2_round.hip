// bk_cnn2_round.hip -- the CNN2 verifier's rounds (bk_roni_cnn2_round_*,
// DESIGN.md §5ad): the forward pass of bk_cnn2.hip, bit for bit, cut for the
// latency of a handful of samples instead of the throughput of thousands.
// k_cnn2 gives a sample to one workgroup, which walks the sample's conv2 MFMAs
// alone; a verifier's call has 10 samples and 256 CUs.  Here a sample is cut
// into BANDS of bh consecutive rows of the second pooled map, a workgroup of
// four waves is one (sample, band), and the grid is samples x ceil(ph2 / bh).
//
//   staging   as k_cnn2: the evaluation's conv weights, fp32(ww [+ delta]), into
//             LDS (conv2's rows at stride ws, zero past T2), and koff[k], tap k's
//             offset (ci plane, ky row, kx) -- for the BAND's plane stride
//   band map  the LDS holds only the rows of the zero-padded first pooled map
//             that the band's conv2 windows read: padded rows 2 r0 .. 2 r1 + k - 2
//             (r0, r1 the band's rows of the second pooled map), 2 bh + k - 1 of
//             them, times P1w, per channel, at an odd plane stride; and the same
//             slice of the bound operand.  A padded row is zeros where it is the
//             map's own padding (above pooled row 0, below pooled row ph1 - 1); a
//             row that belongs to a neighbouring band is a real pooled row and is
//             computed here too: the halo costs (2 bh + k - 1) / (2 bh) of conv1
//   conv1     VALU, k_cnn2's fp64 tap chains and magnitude chains from a register
//             patch, only for the band's real rows.  A band has few positions (at
//             lfw with bh = 1, 4 x 23), so a lane is (pooled position, share of
//             the c1 channels): position fastest, so a wave's image loads and
//             LDS stores stay contiguous
//   conv2     v_mfma_f64_16x16x4_f64, k_cnn2's step: an item is (row tile of 16
//             output channels, column tile of 4 of the band's pooled positions x
//             4 window elements), round-robin over the waves; k = (ci, ky, kx)
//             ascending, the bound accumulator beside the value's, the pool over
//             the lane quad.  The band's positions are consecutive in the flat
//             feature index, so the quad's first lane stores into the tile's
//             scratch [feature][16 samples] at the band's features
//   fc        a tile is 16 samples of one evaluation; its (population x bands)
//             items count themselves out (grad_last_out) and the last one out
//             runs k_cnn2's two chains over all F features, the verdicts and
//             round_exit.  Nobody waits for anybody.
//
// The begin's consumer stores the sample's flag byte; a score's adds the tile's
// two counts to its update's counters.  The launch's last workgroup out gathers
// the originals' flags through idx, writes the scores and near-tie counts and
// zeroes the counters, as k_cnn_round does.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bk_grad_dev.h"
#include "bk_internal.h"
#include "bk_roni_dev.h"

namespace bk {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int R2_NT = 256;
constexpr int R2_LDS_BYTES = 150 * 1024;  // k_cnn2's dynamic LDS budget: one band of ph2 rows
constexpr int R2_FC = 16;                 // fc steps in flight: 64 features
constexpr int R2_TCNT = 2 * RONI_ROUND_G;             // the tiles' hand-off counters
constexpr int R2_EXIT = R2_TCNT + CNN2_ROUND_TILES;   // the launch's exit counter
static_assert(R2_EXIT + 1 == CNN2_ROUND_CNT_WORDS, "the counters' layout");

// bk.h's fp32_up: not below t
static __device__ __forceinline__ float up32(double t) { return (float)(t * (1.0 + 0x1p-22) + 0x1p-126); }
// the pool's maximum: a NaN in the window stays
static __device__ __forceinline__ float pmax(float a, float b) { return a != a ? a : (b != b || b > a) ? b : a; }

template <int K>
__global__ __launch_bounds__(R2_NT) void k_cnn2_round(const Cnn2RoundLaunch a, const Cnn2Gammas g) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double fb[16];
    __shared__ double eb[CNN2_TS][17];
    __shared__ float lt[CNN2_TS][17];
    __shared__ int64_t srow[CNN2_TS];
    __shared__ unsigned int s_cons, s_last, s_orig[2 * RONI_ROUND_G];
    const Cnn2Dims &m = a.m;
    const int tid = threadIdx.x, l = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = m.C, c1 = m.c1, c2 = m.c2, T1 = m.T1, T2 = m.T2, P1w = m.P1w;
    const int64_t F = m.F;
    const bool begin = a.g == 0;
    const int bh = a.bh, nbd = (m.ph2 + bh - 1) / bh;
    const int bps = cnn2_band_stride(m, bh);
    float *const A1 = lds, *const Q1 = A1 + c1 * bps, *const W2s = Q1 + c1 * bps,
                 *const W1s = W2s + c2 * m.ws, *const B1 = W1s + c1 * T1, *const B2 = B1 + c1;
    int *const koff = (int *)(B2 + c2);

    // the workgroup's sample (evaluation q, position p), its tile's slot in the launch, its band
    const unsigned int smp = blockIdx.x / (unsigned int)nbd;
    const int band = (int)(blockIdx.x - smp * (unsigned int)nbd);
    const int64_t total = begin ? a.nv : a.nb, tpe = (total + CNN2_TS - 1) / CNN2_TS;
    const int64_t gs = a.samp_lo + (int64_t)smp;
    const int q = (int)(gs / total);
    const int64_t p = gs - (int64_t)q * total;
    const int64_t p0 = p & ~(int64_t)(CNN2_TS - 1);  // the tile's first sample
    const int col = (int)(p - p0);
    const int slot = (int)((int64_t)q * tpe + p0 / CNN2_TS - (int64_t)a.tile_lo);
    const unsigned int pop = (unsigned int)(total - p0 < CNN2_TS ? total - p0 : CNN2_TS);
    const int r0 = band * bh, r1 = r0 + bh < m.ph2 ? r0 + bh : m.ph2;  // rows of the second pooled map
    const double *__restrict__ ww = a.ww;
    const double *__restrict__ dj = begin ? nullptr : a.rows.p[q];
    auto index = [&](int64_t i) { return a.idx_dev ? a.idx_dev[i] : (int64_t)a.idx_arg.v[i]; };
    auto sample = [&](int64_t pq) {  // position pq of the evaluation: its row in the set
        int64_t row = begin ? pq : index((int64_t)(2 * q + 1) * a.nb + pq);
        if (row < 0 || row >= a.nv) row = 0;  // the host entry has refused it; never out of range
        return row;
    };
    // entry i of the evaluation's model, as torch.FloatTensor holds it
    auto model = [&](int64_t i) { return (float)(dj ? ww[i] + dj[i] : ww[i]); };
    const int64_t o_b1 = (int64_t)c1 * T1, o_w2 = o_b1 + c1, o_b2 = o_w2 + (int64_t)c2 * T2,
                  o_fw = o_b2 + c2, o_fb = o_fw + (int64_t)C * F;

    for (int i = tid; i < c1 * T1; i += R2_NT) W1s[i] = model(i);
    for (int i = tid; i < c1; i += R2_NT) B1[i] = model(o_b1 + i);
    for (int i = tid; i < c2; i += R2_NT) B2[i] = model(o_b2 + i);
    for (int i = tid; i < c2 * m.ws; i += R2_NT) {
        const int r = i / m.ws, k = i - r * m.ws;
        W2s[i] = k < T2 ? model(o_w2 + (int64_t)r * T2 + k) : 0.0f;
    }
    for (int k = tid; k < 4 * m.st2; k += R2_NT) {
        const int ci = k / (K * K), t = k - ci * (K * K), ky = t / K, kx = t - ky * K;
        koff[k] = k < T2 ? ci * bps + ky * P1w + kx : 0;
    }
    for (int i = tid; i < 2 * c1 * bps; i += R2_NT) A1[i] = 0.0f;  // A1 and Q1: the padding stays zero
    __syncthreads();

    // ---- conv1, ReLU, pool for the band's real rows: lane = (pooled position, channel share).
    // Padded row pr of the map is pooled row pr - pad; the band holds padded rows
    // 2 r0 .. 2 r1 + K - 2, local row = pr - 2 r0
    {
        const int pr_lo = 2 * r0 > m.pad ? 2 * r0 : m.pad;
        const int pr_top = 2 * r1 + K - 2, pr_end = m.pad + m.ph1 - 1;
        const int pr_hi = pr_top < pr_end ? pr_top : pr_end;
        const int npos = (pr_hi - pr_lo + 1) * m.pw1;  // <= 0: nothing real (never for a valid shape)
        int nsh = npos > 0 ? R2_NT / npos : 1;
        nsh = nsh < 1 ? 1 : nsh > c1 ? c1 : nsh;
        const int cps = (c1 + nsh - 1) / nsh;  // channels per share
        const float *__restrict__ img = a.X + sample(p) * ((int64_t)m.c_in * m.h * m.w);
        const int hw = m.h * m.w;
        for (int wi = tid; wi < npos * nsh; wi += R2_NT) {
            const int sh = wi / npos, pos = wi - sh * npos;
            const int ry = pos / m.pw1, px = pos - ry * m.pw1;
            const int py = pr_lo - m.pad + ry;  // the pooled row in the map
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
            const int o = (pr_lo + ry - 2 * r0) * P1w + px + m.pad;
            const int c_hi = (sh + 1) * cps < c1 ? (sh + 1) * cps : c1;
#pragma unroll 1
            for (int c = sh * cps; c < c_hi; ++c) {
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
                A1[c * bps + o] = av;
                Q1[c * bps + o] = up32(g.g2 * (double)av + g.h2 * (double)tv);
            }
        }
    }
    __syncthreads();

    // ---- conv2 on the MFMA, ReLU, pool, into the tile's scratch at the band's features
    const int s16 = l & 15, q4 = l >> 4;
    float *const sa = a.scratch + (size_t)slot * cnn2_tile_floats(m);
    float *const sb = sa + (size_t)m.F4 * CNN2_TS;
    {
        const int nbp = (r1 - r0) * m.pw2;  // the band's pooled positions, pp0 + [0, nbp) in the map
        const int pp0 = r0 * m.pw2;
        const int nrt = (c2 + 15) >> 4, nct = (nbp + 3) >> 2;
#pragma unroll 1
        for (int item = wave; item < nrt * nct; item += R2_NT / 64) {
            const int ct = item / nrt, rt = item - ct * nrt;
            const int pl = 4 * ct + (s16 >> 2), plc = pl < nbp ? pl : 0;
            const int py = plc / m.pw2, px = plc - py * m.pw2;  // py: the row inside the band
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
                if ((s16 & 3) == 0 && c < c2 && pl < nbp) {
                    const size_t e = ((size_t)c * m.np2 + pp0 + pl) * CNN2_TS + col;
                    sa[e] = act;
                    sb[e] = up32(g.gF * (double)act + g.hF * (double)t);
                }
            }
        }
    }
    // the tile's last item out goes on as its consumer and sees the others' stores
    const bool consumer = grad_last_out(a.cnt + R2_TCNT + slot, pop * (unsigned int)nbd, &s_cons);

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
            const int nsteps = (int)(m.F4 >> 2), nch = (nsteps + R2_FC - 1) / R2_FC;
            double wa[R2_FC], wd[R2_FC];
            float bv[R2_FC];
            auto load = [&](int ch) {
#pragma unroll
                for (int st = 0; st < R2_FC; ++st) {
                    const int64_t f = (int64_t)ch * (4 * R2_FC) + 4 * st + q4, fc = f < F ? f : F - 1;
                    wa[st] = ww[arow + fc];
                    wd[st] = dj ? dj[arow + fc] : 0.0;
                    bv[st] = sB[(size_t)fc * CNN2_TS + s16];
                }
            };
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};  // wave 0: the logits; wave 1: the bound
            load(0);
#pragma unroll 1
            for (int ch = 0; ch < nch; ++ch) {
                double av[R2_FC], b[R2_FC];
#pragma unroll
                for (int st = 0; st < R2_FC; ++st) {
                    const bool on = (int64_t)ch * (4 * R2_FC) + 4 * st + q4 < F;
                    const double w = on && con ? (double)(float)(dj ? wa[st] + wd[st] : wa[st]) : 0.0;
                    av[st] = wave ? __builtin_fabs(w) : w;
                    b[st] = on ? (double)bv[st] : 0.0;
                }
                if (ch + 1 < nch) load(ch + 1);  // in flight under this chunk's MFMAs
                const int steps = nsteps - ch * R2_FC < R2_FC ? nsteps - ch * R2_FC : R2_FC;
#pragma unroll
                for (int st = 0; st < R2_FC; ++st)
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
            ok = best == a.y[srow[tid]];
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
            if (begin) a.flags[srow[tid]] = (uint8_t)((ok ? 0 : 1) | (nt ? 2 : 0));
        }
        if (wave == 0) {
            mine[0] = (unsigned int)__popcll(__ballot(ok));
            mine[1] = (unsigned int)__popcll(__ballot(nt));
        }
    }
    if (tid == 0) {
        if (begin) mine[0] = mine[1] = 0u;
        const int where[2] = {2 * q, 2 * q + 1};
        s_last = round_exit(mine, where, a.cnt, R2_EXIT);
    }
    __syncthreads();
    if (!s_last) return;
    // the launch's last workgroup out
    if (a.finish) {
        if (tid < 2 * RONI_ROUND_G) s_orig[tid] = 0u;
        __syncthreads();
        // the originals read no image and no model: the held flags through idx
        for (int64_t i = tid; i < (int64_t)a.g * a.nb; i += R2_NT) {
            const int u = (int)(i / a.nb);
            int64_t row = index((int64_t)(2 * u) * a.nb + (i - (int64_t)u * a.nb));
            if (row < 0 || row >= a.nv) row = 0;
            const unsigned int fl = a.flags[row];
            if (fl & 1u) atomicAdd(&s_orig[2 * u], 1u);
            if (fl & 2u) atomicAdd(&s_orig[2 * u + 1], 1u);
        }
        __syncthreads();
        if (tid < a.g) {
            const unsigned int good1 = round_load(a.cnt + 2 * tid), near1 = round_load(a.cnt + 2 * tid + 1);
            __hip_atomic_store(a.cnt + 2 * tid, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.cnt + 2 * tid + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned int good0 = (unsigned int)(a.nb - (int64_t)s_orig[2 * tid]);
            const double dn = (double)a.nb;
            const double orig = 1.0 - (double)good0 / dn, after = 1.0 - (double)good1 / dn;
            a.scores[tid] = after - orig;
            a.near[2 * tid] = (int32_t)s_orig[2 * tid + 1];
            a.near[2 * tid + 1] = (int32_t)near1;
        }
    }
    if (tid == 0) __hip_atomic_store(a.cnt + R2_EXIT, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int K>
static hipError_t launch_k(const Cnn2RoundLaunch &a, unsigned int grid, int lds, hipStream_t st) {
    // per device, so asked on every launch: a tall band exceeds the default 64 KiB
    const hipError_t e = hipFuncSetAttribute((const void *)k_cnn2_round<K>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, R2_LDS_BYTES);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cnn2_round<K>, dim3(grid), dim3(R2_NT), (size_t)lds, st, a, cnn2_gammas(a.m));
    return hipGetLastError();
}

hipError_t launch_cnn2_round(const Cnn2RoundLaunch &in, hipStream_t st) {
    Cnn2RoundLaunch a = in;
    const Cnn2Dims &m = a.m;
    if (a.tiles < 1 || a.tiles > CNN2_ROUND_TILES || a.tile_lo < 0 || a.bh < 1 || a.bh > m.ph2 ||
        a.g < 0 || a.g > RONI_ROUND_G || m.k < 1 || m.k > 3 || m.c_in < 1 || m.c_in > 3 ||
        !a.scratch || !a.cnt || !a.flags)
        return hipErrorInvalidConfiguration;
    const int lds = cnn2_band_lds(m, a.bh);
    const int64_t total = a.g ? a.nb : a.nv;
    if (total < 1 || lds < 1 || lds > R2_LDS_BYTES) return hipErrorInvalidConfiguration;
    const int64_t tpe = cnn2_tiles(total), space = (int64_t)(a.g ? a.g : 1) * tpe;
    if ((int64_t)a.tile_lo + a.tiles > space) return hipErrorInvalidConfiguration;
    // the samples of the space before tile T = e tpe + t: e total + min(16 t, total)
    auto before = [&](int64_t T) {
        const int64_t e = T / tpe, t = T - e * tpe;
        return e * total + (t * CNN2_TS < total ? t * CNN2_TS : total);
    };
    a.samp_lo = before(a.tile_lo);
    const int64_t samples = before((int64_t)a.tile_lo + a.tiles) - a.samp_lo;
    const unsigned int grid = (unsigned int)samples * (unsigned int)((m.ph2 + a.bh - 1) / a.bh);
    switch (m.k) {
    case 1: return launch_k<1>(a, grid, lds, st);
    case 2: return launch_k<2>(a, grid, lds, st);
    default: return launch_k<3>(a, grid, lds, st);
    }
}

}  // namespace bk
