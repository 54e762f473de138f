// bk_cnn_round.hip -- the CNN verifier's rounds (bk_roni_cnn_round_*, DESIGN.md
// §5aa): the forward pass of bk_cnn.hip, bit for bit, cut for the latency of
// ONE tile instead of the throughput of hundreds.  k_cnn keeps a tile's
// convolution and its two fc chains in one workgroup, the chain wave waiting at
// every chunk barrier for four producer waves; here the convolution leaves the
// chains' critical path and spreads over the grid.
//
// One launch, two kinds of work:
//
//   conv item  (tile of <= 16 samples, range of rc ring chunks of 64 features).
//              The workgroup stages the tile's images into LDS as k_cnn's
//              zero-padded planes (stride 4 mod 64 words) and the evaluation's
//              conv weights and biases as doubles of fp32(ww [+ delta]).  Lane
//              (sg = l & 3, fq = l >> 2) of wave w runs feature 64 ch + 16 w + fq
//              of samples 4 sg .. 4 sg + 3: a wave's 64 lanes read 64 different
//              banks per tap (4 (4 sg + i) + fq), a tap's weight is read once
//              for four samples, and the lane stores the four activations and
//              the four bound operands with one 16-byte store each into the
//              tile's scratch -- per feature the 16 samples contiguous, the
//              MFMA's B operand as the chains read it.
//   chain      one per tile.  The conv items of a tile count themselves out on
//              the tile's counter (plain stores, release fence, counter: grad_
//              last_out); the one that leaves last goes on as the tile's
//              consumer.  Nobody waits for anybody.  Wave 0 runs the logits'
//              chain and wave 1 the bound's, one dependent
//              v_mfma_f64_16x16x4_f64 per 4 features each; waves 2 and 3 load:
//              they stream the fc weights (and the delta) from L2 two chunks
//              ahead in registers, round fp32(ww + delta) once and put it into
//              a two-slot LDS ring as the A operand (16 class rows, rows past C
//              zero, row stride 68 doubles: 2 lanes per bank pair), and copy
//              the scratch's B chunks into the ring beside it.  The chain waves
//              issue no global load.  One barrier per chunk.
//
// Lane s of wave 0 takes argmax, label compare and near-tie test of sample s
// (k_cnn's expressions).  The begin's consumer stores the sample's flag byte;
// a score's adds the tile's two counts to its update's counters.  The launch's
// last workgroup out (round_exit) gathers the originals' flags through idx,
// writes the scores and near-tie counts and zeroes the counters.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bk_grad_dev.h"
#include "bk_internal.h"
#include "bk_roni_dev.h"

namespace bk {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int CR_NT = 256;                // 4 waves: conv lanes; then 2 chains + 2 loaders
constexpr int CR_KC = CNN_ROUND_KC;       // features per ring chunk
constexpr int CR_TS = 16;                 // the MFMA's columns
constexpr int CR_AS = CR_KC + 4;          // A's row stride in the ring (doubles)
constexpr int CR_IMG_BYTES = 96 * 1024;   // the planes' LDS budget (bk_cnn.hip's)
constexpr int CR_MAX_CO = 16;
constexpr int CR_TCNT = 2 * RONI_ROUND_G;             // the tiles' hand-off counters
constexpr int CR_EXIT = CR_TCNT + CNN_ROUND_TILES;    // the launch's exit counter
static_assert(CR_EXIT + 1 == CNN_ROUND_CNT_WORDS, "the counters' layout");

// a loader lane's share of one chunk in flight: 8 class rows of one feature
// (weights and delta), 2 + 2 quads of the scratch's activations and bounds
struct CrStage {
    double w[8], d[8];
    float4 b[4];
};

template <int K>
__global__ __launch_bounds__(CR_NT) void k_cnn_round(const CnnRoundLaunch a, double gF, double ge) {
    extern __shared__ __attribute__((aligned(16))) float img[];  // ts planes of ps words
    __shared__ __attribute__((aligned(16))) double As[2][16][CR_AS];
    __shared__ __attribute__((aligned(16))) float Bs[2][2][CR_KC][CR_TS];  // [slot][activation, bound]
    __shared__ double cw[CR_MAX_CO * K * K], cb[CR_MAX_CO], fb[16];
    __shared__ double eb[CR_TS][17];
    __shared__ float lt[CR_TS][17];
    __shared__ int64_t srow[CR_TS];
    __shared__ unsigned int s_cons, s_last, s_orig[2 * RONI_ROUND_G];
    const CnnDims &m = a.m;
    const int tid = threadIdx.x, l = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = m.C, ts = m.ts;
    const int64_t F = m.F;
    const bool begin = a.g == 0;
    const int nch = cnn_round_chunks(m);
    const int R = (nch + a.rc - 1) / a.rc;  // conv items per tile

    // the workgroup's tile (slot: its place in the launch), item and model
    const int slot = (int)(blockIdx.x / (unsigned)R), item = (int)blockIdx.x - slot * R;
    const int64_t total = begin ? a.nv : a.nb;
    const int tpe = cnn_tiles(m, total);
    const int T = a.tile_lo + slot, q = T / tpe;
    const int64_t p0 = (int64_t)(T - q * tpe) * ts;
    const double *__restrict__ ww = a.ww;
    const double *__restrict__ dj = begin ? nullptr : a.rows.p[q];
    auto index = [&](int64_t i) { return a.idx_dev ? a.idx_dev[i] : (int64_t)a.idx_arg.v[i]; };
    // entry i of the evaluation's model, as torch.FloatTensor holds it
    auto model = [&](int64_t i) { return (double)(float)(dj ? ww[i] + dj[i] : ww[i]); };
    const int64_t o_cb = (int64_t)m.co * K * K, o_fw = o_cb + m.co, o_fb = o_fw + (int64_t)C * F;

    for (int i = tid; i < m.co * K * K; i += CR_NT) cw[i] = model(i);
    if (tid < CR_MAX_CO) cb[tid] = tid < m.co ? model(o_cb + tid) : 0.0;
    if (tid >= 64 && tid < 80) fb[tid - 64] = tid - 64 < C ? model(o_fb + tid - 64) : 0.0;
    if (tid >= 128 && tid < 128 + CR_TS) {  // the tile's rows; -1: no sample
        const int s = tid - 128;
        int64_t row = -1;
        if (s < ts && p0 + s < total) {
            row = begin ? p0 + s : index((int64_t)(2 * q + 1) * a.nb + p0 + s);
            if (row < 0 || row >= a.nv) row = 0;  // the host entry has refused it; never out of range
        }
        srow[s] = row;
    }
    __syncthreads();
    {
        const int plane = m.ph * m.pw;
        const int64_t ldv = (int64_t)m.h * m.w;
        for (int i = tid; i < ts * plane; i += CR_NT) {
            const int s = i / plane, r = i - s * plane, yy = r / m.pw, xx = r - yy * m.pw;
            const int64_t row = srow[s];
            const bool in = row >= 0 && yy >= m.pad && yy < m.pad + m.h && xx >= m.pad && xx < m.pad + m.w;
            img[s * m.ps + r] = in ? a.X[row * ldv + (int64_t)(yy - m.pad) * m.w + (xx - m.pad)] : 0.0f;
        }
    }
    __syncthreads();

    // ---- the conv item: chunks [item rc, item rc + rc) of the tile into the scratch
    const size_t half = (size_t)nch * CR_KC * CR_TS;
    float *__restrict__ sa = a.scratch + (size_t)slot * 2 * half;
    float *__restrict__ sb = sa + half;
    {
        const int sg = l & 3, fq = l >> 2;
        const unsigned plane_o = (unsigned)(m.oh * m.ow);
        int so[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) so[i] = (4 * sg + i < ts ? 4 * sg + i : 0) * m.ps;
        const int c_hi = (item + 1) * a.rc < nch ? (item + 1) * a.rc : nch;
#pragma unroll 1
        for (int ch = item * a.rc; ch < c_hi; ++ch) {
            const int64_t f = (int64_t)ch * CR_KC + 16 * wave + fq;
            float av[4] = {0.0f, 0.0f, 0.0f, 0.0f}, tv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (f < F) {
                const unsigned fu = (unsigned)f, c = fu / plane_o, r = fu - c * plane_o,
                               y = r / (unsigned)m.ow, x = r - y * (unsigned)m.ow;
                const float *px = img + y * m.pw + x;
                const double *pw = cw + c * (K * K);
                double acc[4] = {0.0, 0.0, 0.0, 0.0}, mag[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int ky = 0; ky < K; ++ky)
#pragma unroll
                    for (int kx = 0; kx < K; ++kx) {
                        const double wv = pw[ky * K + kx], aw = __builtin_fabs(wv);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const double xv = (double)px[so[i] + ky * m.pw + kx];
                            acc[i] = __builtin_fma(xv, wv, acc[i]);
                            mag[i] = __builtin_fma(__builtin_fabs(xv), aw, mag[i]);
                        }
                    }
                const double bias = cb[c];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float pre = (float)(acc[i] + bias);
                    const float act = pre < 0.0f ? 0.0f : pre;  // a NaN stays
                    const double t = gF * (double)act + ge * (mag[i] + __builtin_fabs(bias));
                    if (4 * sg + i < ts) {
                        av[i] = act;
                        tv[i] = (float)(t * (1.0 + 0x1p-22) + 0x1p-126);  // rounded up
                    }
                }
            }
            // features past F and samples past ts are zeros: the chains' tails
            *(float4 *)(sa + (size_t)f * CR_TS + 4 * sg) = make_float4(av[0], av[1], av[2], av[3]);
            *(float4 *)(sb + (size_t)f * CR_TS + 4 * sg) = make_float4(tv[0], tv[1], tv[2], tv[3]);
        }
    }
    // the tile's last item out goes on as its consumer and sees the others' stores
    const bool consumer = grad_last_out(a.cnt + CR_TCNT + slot, (unsigned)R, &s_cons);

    unsigned int mine[2] = {0u, 0u};
    if (consumer) {
        const int s16 = l & 15, q4 = l >> 4;
        const int t = tid - 128, lf = t & 63, cg = t >> 6;  // a loader lane's feature and class parity
        const float4 *__restrict__ ga = (const float4 *)sa, *__restrict__ gb = (const float4 *)sb;
        auto issue = [&](CrStage &S, int ch) {
            const int64_t f = (int64_t)ch * CR_KC + lf;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int c = cg + 2 * i;
                const bool on = ch < nch && f < F && c < C;
                const int64_t e = o_fw + (int64_t)c * F + f;
                S.w[i] = on ? ww[e] : 0.0;
                S.d[i] = on && dj ? dj[e] : 0.0;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const size_t e = (size_t)ch * (CR_KC * CR_TS / 4) + t + 128 * (i & 1);
                S.b[i] = ch < nch ? (i < 2 ? ga[e] : gb[e]) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        };
        auto commit = [&](const CrStage &S, int rs) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                As[rs][cg + 2 * i][lf] = (double)(float)(dj ? S.w[i] + S.d[i] : S.w[i]);
#pragma unroll
            for (int i = 0; i < 4; ++i) ((float4 *)Bs[rs][i >> 1])[t + 128 * (i & 1)] = S.b[i];
        };
        d4 acc = d4{0.0, 0.0, 0.0, 0.0};  // wave 0: the logits; wave 1: the bound
        auto consume = [&](int ch, int rs) {
            const int64_t left = F - (int64_t)ch * CR_KC;
            const int steps = left < CR_KC ? (int)((left + 3) >> 2) : CR_KC / 4;
#pragma unroll
            for (int st = 0; st < CR_KC / 4; ++st) {
                if (st < steps) {
                    const double w = As[rs][s16][4 * st + q4];
                    const double b = (double)Bs[rs][wave][4 * st + q4][s16];
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wave ? __builtin_fabs(w) : w, b, acc, 0, 0, 0);
                }
            }
        };
        CrStage S0, S1;  // chunk c is in flight in stage c & 1 and lands in ring slot c & 1
        if (wave >= 2) {
            issue(S0, 0);
            issue(S1, 1);
            commit(S0, 0);
            issue(S0, 2);
        }
        __syncthreads();
#pragma unroll 1
        for (int ch = 0; ch < nch; ch += 2) {
            if (wave >= 2) {
                commit(S1, 1);
                issue(S1, ch + 3);
            } else {
                consume(ch, 0);
            }
            __syncthreads();
            if (wave >= 2) {
                commit(S0, 0);
                issue(S0, ch + 4);
            } else if (ch + 1 < nch) {
                consume(ch + 1, 1);
            }
            __syncthreads();
        }
        if (wave < 2) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = q4 + 4 * r;
                if (wave == 0)
                    lt[s16][c] = (float)(acc[r] + fb[c]);
                else
                    eb[s16][c] = acc[r] + gF * __builtin_fabs(fb[c]);
            }
        }
        __syncthreads();
        bool ok = false, nt = false;
        const bool have = tid < CR_TS && srow[tid < CR_TS ? tid : 0] >= 0;
        if (have) {
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
        s_last = round_exit(mine, where, a.cnt, CR_EXIT);
    }
    __syncthreads();
    if (!s_last) return;
    // the launch's last workgroup out
    if (a.finish) {
        if (tid < 2 * RONI_ROUND_G) s_orig[tid] = 0u;
        __syncthreads();
        // the originals read no image and no model: the held flags through idx
        for (int64_t i = tid; i < (int64_t)a.g * a.nb; i += CR_NT) {
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
    if (tid == 0) __hip_atomic_store(a.cnt + CR_EXIT, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int K>
static hipError_t launch_k(const CnnRoundLaunch &a, unsigned grid, double gF, double ge, hipStream_t st) {
    // per device, so asked on every launch: the planes exceed the default 64 KiB
    const hipError_t e = hipFuncSetAttribute((const void *)k_cnn_round<K>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, CR_IMG_BYTES);
    if (e != hipSuccess) return e;
    const size_t lds = (size_t)a.m.ts * a.m.ps * sizeof(float);
    hipLaunchKernelGGL(k_cnn_round<K>, dim3(grid), dim3(CR_NT), lds, st, a, gF, ge);
    return hipGetLastError();
}

hipError_t launch_cnn_round(const CnnRoundLaunch &a, hipStream_t st) {
    const CnnDims &m = a.m;
    const int nch = cnn_round_chunks(m);
    if (a.tiles < 1 || a.tiles > CNN_ROUND_TILES || a.tile_lo < 0 || a.rc < 1 || a.rc > nch ||
        a.g < 0 || a.g > RONI_ROUND_G || m.ts < 1 || m.ts > CR_TS || m.k < 1 || m.k > 5 ||
        m.co > CR_MAX_CO || (size_t)m.ts * m.ps * sizeof(float) > CR_IMG_BYTES)
        return hipErrorInvalidConfiguration;
    const int64_t total = a.g ? a.nb : a.nv;
    const int64_t space = (int64_t)(a.g ? a.g : 1) * cnn_tiles(m, total);
    if (total < 1 || (int64_t)a.tile_lo + a.tiles > space) return hipErrorInvalidConfiguration;
    const unsigned grid = (unsigned)a.tiles * (unsigned)((nch + a.rc - 1) / a.rc);
    double gF, ge;
    cnn_gammas(m, &gF, &ge);
    switch (m.k) {
    case 1: return launch_k<1>(a, grid, gF, ge, st);
    case 2: return launch_k<2>(a, grid, gF, ge, st);
    case 3: return launch_k<3>(a, grid, gF, ge, st);
    case 4: return launch_k<4>(a, grid, gF, ge, st);
    default: return launch_k<5>(a, grid, gF, ge, st);
    }
}

}  // namespace bk
