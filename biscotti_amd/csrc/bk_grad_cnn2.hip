// bk_grad_cnn2.hip -- the gradient step of the two-layer lfw CNN (bk.h
// bk_grad_cnn2), gfx950: the backward half of the model k_cnn2
// (bk_cnn2.hip) scores, on the peer's resident shard.  Client.getGrad
// (ML/Pytorch/client.py:38-65) on LFWCNNModel, negated (client_obj.py:73-77),
// and the quantisation behind it (updateFloatToInt).
//
//   k_grad_cnn2_fwd  one workgroup per batch position.  conv1 and its pool on
//                    the VALU from a register patch, conv2 on
//                    v_mfma_f64_16x16x4_f64 with the pool across the lane quad,
//                    both exactly k_cnn2's values without its bound planes;
//                    each pool keeps the 2-bit code of its first maximum.  The
//                    logits are 256 lane chains over the features and a fixed
//                    tree; then the softmax, r, the loss part and g2.  A1's
//                    padded planes, both code maps, A2, g2 and r go to the
//                    position's scratch: the maps are not computed again
//   k_grad_cnn2_bwd  grid = positions x items, so that the deployed batch of 10
//                    fills the device.  A W2 item is a column tile of 16 conv2
//                    taps (the conv2 bias rides as a column held at 1 behind
//                    the last tap): dP2 (g2 where the code selects the window
//                    element) times the A1 planes the taps touch, staged in
//                    LDS zero-padded, k = the kept conv2 positions, pooled
//                    position pp in wave pp mod 4, the waves' sums added in
//                    wave order.  A D1 item is a band of two pooled-1 rows:
//                    dA1 = conv2's weights (rows ci, k = (co, ky, kx)) times
//                    the band's zero-padded dP2, masked by A1 > 0 into LDS;
//                    then the band's share of Gw1 / Gb1, dP1 (dA1 where pool
//                    1's code selects) times the band's zero-padded input rows,
//                    one wave per 16 x 16 tile of (c1, taps + bias), its
//                    accumulators in registers across the band
//   k_grad_cnn2_sum  per gradient entry: the parts over positions ascending
//                    (a position's items ascending), GW and gb as chains over
//                    the positions; / N; the last workgroup out takes the loss,
//                    the norm and coef
//   k_grad_cnn2_tail clip, negate, add the noise, quantise, store
//
// Nobody waits for anybody (grad_last_out); every sum has one fixed order,
// whatever the grid or the timing.  Built with -ffp-contract=off: only the
// chains are FMAs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bk_ctx.h"
#include "bk_grad_dev.h"

namespace bk {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));
typedef long long ll2 __attribute__((ext_vector_type(2)));
typedef unsigned char u8;

constexpr int GC2_NT = 256;
constexpr int GC2_BH = 2;                 // pooled-1 rows of a D1 item
constexpr int GC2_LDS = 128 * 1024;       // the dynamic LDS budget; the static arrays come on top
constexpr int GC2_MAX_RT2 = 3, GC2_MAX_RT1 = 2;  // row tiles of c2 <= 48, of c1 <= 32

static int64_t up16(int64_t v) { return (v + 15) / 16 * 16; }

// bk.h's formula and the scratch layout
bool grad_cnn2_plan(const Cnn2Dims &m, GradCnn2Plan *out) {
    GradCnn2Plan p = {};
    const int K = m.k, KK = K * K;
    p.nw2 = (m.T2 + 1 + 15) / 16;
    p.nrt2 = (m.c2 + 15) / 16;
    p.npl = 15 / KK + 2 < m.c1 ? 15 / KK + 2 : m.c1;
    p.nd1 = (m.ph1 + GC2_BH - 1) / GC2_BH;
    p.nrt1 = (m.c1 + 15) / 16;
    p.bw = m.pw1 + K - 1;
    p.dps = ((GC2_BH + K - 1) * p.bw) | 1;
    p.nbm = GC2_BH * m.pw1;
    p.xw = 2 * m.pw1 + K - 1;
    p.xrows = 2 * GC2_BH + K - 1;
    p.xps = p.xrows * p.xw;
    const int64_t F = m.F;
    const int64_t fwd = 4 * ((int64_t)m.c1 * m.ps1 + (int64_t)m.c2 * m.ws + m.c1 * m.T1 + m.c1 + m.c2 +
                             4 * m.st2 + F);
    const int64_t w2 = up16(8 * F + 4 * (int64_t)p.npl * m.ps1 + F);
    const int64_t d1 = up16(8 * ((int64_t)m.c2 * p.dps + 16 * p.nrt1 * p.nbm) +
                            4 * ((int64_t)m.c2 * m.T2 + m.c_in * p.xps) + 16 * p.nrt1 * p.nbm);
    if (fwd > GC2_LDS || w2 > GC2_LDS || d1 > GC2_LDS) return false;
    p.lds_fwd = (int)fwd;
    p.lds_bwd = (int)(w2 > d1 ? w2 : d1);
    p.o_pw2 = 8 * F;
    p.o_pd1 = p.o_pw2 + 8 * (int64_t)p.nw2 * 16 * p.nrt2 * 16;
    p.o_r = p.o_pd1 + 8 * (int64_t)p.nd1 * 16 * p.nrt1 * 32;
    p.o_a1 = p.o_r + 8 * 18;  // r (16), the loss part, a spare
    p.o_a2 = p.o_a1 + up16(4 * (int64_t)m.c1 * m.ps1);
    p.o_c1 = p.o_a2 + up16(4 * F);
    p.o_c2 = p.o_c1 + up16((int64_t)m.c1 * m.ph1 * m.pw1);
    p.stride = (p.o_c2 + up16(F) + 255) / 256 * 256;
    *out = p;
    return true;
}

// the row of the resident set behind batch position s
__device__ __forceinline__ int64_t gc2_row(const GradCnn2Args &a, int64_t s) {
    int64_t row = a.rows ? a.rows[s] : s;
    if (row < 0 || row >= a.nn) row = 0;  // the host entry has refused it; never out of range
    return row;
}

template <int K>
__global__ __launch_bounds__(GC2_NT) void k_grad_cnn2_fwd(const GradCnn2Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double red[GRAD_TILE];
    __shared__ double lgs[16], rsh[16];
    const Cnn2Dims &m = a.m;
    const int tid = threadIdx.x, l = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = m.C, c1 = m.c1, c2 = m.c2, T1 = m.T1, T2 = m.T2, ps1 = m.ps1, P1w = m.P1w;
    const int np1 = m.ph1 * m.pw1, np2 = m.np2;
    const int64_t F = m.F;
    float *const A1 = lds, *const W2s = A1 + c1 * ps1, *const W1s = W2s + c2 * m.ws,
                 *const B1 = W1s + c1 * T1, *const B2 = B1 + c1;
    int *const koff = (int *)(B2 + c2);
    float *const A2 = (float *)(koff + 4 * m.st2);
    const int64_t s = (int64_t)blockIdx.x, row = gc2_row(a, s);
    char *const scr = a.scr + s * a.p.stride;
    double *const g2g = (double *)scr, *const rg = (double *)(scr + a.p.o_r);
    float *const A1g = (float *)(scr + a.p.o_a1), *const A2g = (float *)(scr + a.p.o_a2);
    u8 *const c1g = (u8 *)(scr + a.p.o_c1), *const c2g = (u8 *)(scr + a.p.o_c2);
    const double *__restrict__ ww = a.ww;
    const int64_t o_b1 = (int64_t)c1 * T1, o_w2 = o_b1 + c1, o_b2 = o_w2 + (int64_t)c2 * T2,
                  o_fw = o_b2 + c2, o_fb = o_fw + (int64_t)C * F;

    for (int i = tid; i < c1 * T1; i += GC2_NT) W1s[i] = (float)ww[i];
    for (int i = tid; i < c1; i += GC2_NT) B1[i] = (float)ww[o_b1 + i];
    for (int i = tid; i < c2; i += GC2_NT) B2[i] = (float)ww[o_b2 + i];
    for (int i = tid; i < c2 * m.ws; i += GC2_NT) {
        const int r = i / m.ws, k = i - r * m.ws;
        W2s[i] = k < T2 ? (float)ww[o_w2 + (int64_t)r * T2 + k] : 0.0f;
    }
    for (int k = tid; k < 4 * m.st2; k += GC2_NT) {
        const int ci = k / (K * K), t = k - ci * (K * K), ky = t / K, kx = t - ky * K;
        koff[k] = k < T2 ? ci * ps1 + ky * P1w + kx : 0;
    }
    for (int i = tid; i < c1 * ps1; i += GC2_NT) A1[i] = 0.0f;  // the borders stay zero
    __syncthreads();

    // ---- conv1, ReLU, pool and its code: lane = pooled position, all channels
    {
        const float *__restrict__ img = a.X + row * ((int64_t)m.c_in * m.h * m.w);
        const int hw = m.h * m.w;
        for (int pos = tid; pos < np1; pos += GC2_NT) {
            const int py = pos / m.pw1, px = pos - py * m.pw1;
            double x[3][K + 1][K + 1];
#pragma unroll
            for (int ci = 0; ci < 3; ++ci)
#pragma unroll
                for (int r = 0; r <= K; ++r)
#pragma unroll
                    for (int q = 0; q <= K; ++q) {
                        const int iy = 2 * py - m.pad + r, ix = 2 * px - m.pad + q;
                        const bool in = ci < m.c_in && iy >= 0 && iy < m.h && ix >= 0 && ix < m.w;
                        x[ci][r][q] = in ? (double)img[ci * hw + iy * m.w + ix] : 0.0;
                    }
            const int o = (py + m.pad) * P1w + px + m.pad;
#pragma unroll 1
            for (int c = 0; c < c1; ++c) {
                const float *pw = W1s + c * T1;
                double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int ci = 0; ci < 3; ++ci)
                    if (ci < m.c_in) {
#pragma unroll
                        for (int ky = 0; ky < K; ++ky)
#pragma unroll
                            for (int kx = 0; kx < K; ++kx) {
                                const double wv = (double)pw[(ci * K + ky) * K + kx];
#pragma unroll
                                for (int e = 0; e < 4; ++e)
                                    acc[e] = __builtin_fma(x[ci][ky + (e >> 1)][kx + (e & 1)], wv, acc[e]);
                            }
                    }
                const double bias = (double)B1[c];
                float av = 0.0f;
                int code = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float pre = (float)(acc[e] + bias);
                    const float act = pre < 0.0f ? 0.0f : pre;  // a NaN stays
                    const bool take = e == 0 || (!(av != av) && (act != act || act > av));  // the first maximum
                    av = take ? act : av;
                    code = take ? e : code;
                }
                A1[c * ps1 + o] = av;
                c1g[c * np1 + pos] = (u8)code;
            }
        }
    }
    __syncthreads();

    // ---- conv2 on the MFMA, ReLU, pool and its code
    const int s16 = l & 15, q4 = l >> 4;
    {
        const int nrt = (c2 + 15) >> 4, nct = (np2 + 3) >> 2;
#pragma unroll 1
        for (int item = wave; item < nrt * nct; item += GC2_NT / 64) {
            const int ct = item / nrt, rt = item - ct * nrt;
            const int pp = 4 * ct + (s16 >> 2), ppc = pp < np2 ? pp : 0;
            const int py = ppc / m.pw2, px = ppc - py * m.pw2;
            const int pbase = (2 * py + ((s16 >> 1) & 1)) * P1w + 2 * px + (s16 & 1);
            const int arow = 16 * rt + s16;
            const bool aon = arow < c2;
            const float *wrow = W2s + (aon ? arow : 0) * m.ws;
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
            for (int st = 0; st < m.st2; ++st) {
                const int k = 4 * st + q4;
                const double wv = aon ? (double)wrow[k] : 0.0;  // zero past T2
                const double b = k < T2 ? (double)A1[koff[k] + pbase] : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wv, b, acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = 16 * rt + q4 + 4 * r;
                const float pre = (float)(acc[r] + (double)B2[c < c2 ? c : 0]);
                const float act = pre < 0.0f ? 0.0f : pre;  // a NaN stays
                float av = 0.0f;
                int code = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {  // the quad's four window elements, (dy, dx) ascending
                    const float v = __shfl(act, (l & ~3) | e);
                    const bool take = e == 0 || (!(av != av) && (v != v || v > av));
                    av = take ? v : av;
                    code = take ? e : code;
                }
                if ((s16 & 3) == 0 && c < c2 && pp < np2) {
                    A2[c * np2 + pp] = av;
                    c2g[c * np2 + pp] = (u8)code;
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < c1 * ps1; i += GC2_NT) A1g[i] = A1[i];
    for (int i = tid; i < (int)F; i += GC2_NT) A2g[i] = A2[i];

    // ---- the logits: lane chains over f = tid, tid + 256, .., then the tree, then the bias
    for (int c = 0; c < C; ++c) {
        double acc = 0.0;
        for (int f = tid; f < (int)F; f += GC2_NT)
            acc = __builtin_fma((double)(float)ww[o_fw + (int64_t)c * F + f], (double)A2[f], acc);
        const double v = grad_tree(red, acc);
        if (tid == 0) lgs[c] = v + (double)(float)ww[o_fb + c];
    }
    __syncthreads();
    if (tid == 0) {  // bk_grad_softmax's rule
        int yy = a.y[row];
        yy = yy < 0 || yy >= C ? 0 : yy;
        double mx = lgs[0];
        for (int c = 1; c < C; ++c) mx = lgs[c] > mx ? lgs[c] : mx;
        double sum = 0.0;
        for (int c = 0; c < C; ++c) {
            const double e = exp(lgs[c] - mx);
            rsh[c] = e;
            sum = sum + e;
        }
        for (int c = 0; c < 16; ++c) {
            const double r = c < C ? rsh[c] / sum - (c == yy ? 1.0 : 0.0) : 0.0;
            rsh[c] = r;
            rg[c] = r;
        }
        rg[16] = log(sum) + mx - lgs[yy];
    }
    __syncthreads();
    // ---- g2: the chain over c ascending, masked by the pooled activation
    for (int f = tid; f < (int)F; f += GC2_NT) {
        double acc = 0.0;
        for (int c = 0; c < C; ++c)
            acc = __builtin_fma((double)(float)ww[o_fw + (int64_t)c * F + f], rsh[c], acc);
        const float av = A2[f];
        g2g[f] = av > 0.0f ? acc : (av != av ? (double)av : 0.0);
    }
}

// A W2 item: column tile `tile` of Gw2 | Gb2 for one position
template <int K>
__device__ __forceinline__ void gc2_w2_item(const GradCnn2Args &a, const char *scr, int tile, double *pout,
                                            char *ldsb, double (*wred)[GC2_MAX_RT2][256]) {
    constexpr int KK = K * K;
    const Cnn2Dims &m = a.m;
    const int tid = threadIdx.x, l = tid & 63, s16 = l & 15, kq = l >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c1 = m.c1, c2 = m.c2, T2 = m.T2, ps1 = m.ps1, np2 = m.np2, F = (int)m.F;
    const int nrt = a.p.nrt2, npl = a.p.npl;
    double *const g2s = (double *)ldsb;
    float *const pl = (float *)(ldsb + 8 * (size_t)F);
    u8 *const c2s = (u8 *)(pl + npl * ps1);
    const double *g2g = (const double *)scr;
    const float *A1g = (const float *)(scr + a.p.o_a1);
    const u8 *c2g = (const u8 *)(scr + a.p.o_c2);
    const int t0 = 16 * tile;
    int ci_lo = t0 / KK;
    ci_lo = ci_lo < c1 ? ci_lo : c1 - 1;
    const int nst = c1 - ci_lo < npl ? c1 - ci_lo : npl;
    for (int i = tid; i < F; i += GC2_NT) {
        g2s[i] = g2g[i];
        c2s[i] = c2g[i];
    }
    for (int i = tid; i < nst * ps1; i += GC2_NT) pl[i] = A1g[ci_lo * ps1 + i];
    __syncthreads();
    // the lane's column: a tap, the bias column, or nothing
    const int tcol = t0 + s16, tc = tcol < T2 ? tcol : T2 - 1;
    const int ci = tc / KK, tt = tc - ci * KK, ky = tt / K, kx = tt - ky * K;
    const int boff = (ci - ci_lo) * ps1 + ky * m.P1w + kx + (kq >> 1) * m.P1w + (kq & 1);
    d4 acc[GC2_MAX_RT2];
#pragma unroll
    for (int rt = 0; rt < GC2_MAX_RT2; ++rt) acc[rt] = d4{0.0, 0.0, 0.0, 0.0};
    for (int pp = wave; pp < np2; pp += 4) {
        const int py = pp / m.pw2, px = pp - py * m.pw2;
        const float xv = pl[boff + 2 * py * m.P1w + 2 * px];
        const double bv = tcol < T2 ? (double)xv : tcol == T2 ? 1.0 : 0.0;
#pragma unroll
        for (int rt = 0; rt < GC2_MAX_RT2; ++rt)
            if (rt < nrt) {
                const int co = 16 * rt + s16, e = (co < c2 ? co : 0) * np2 + pp;
                const double gv = g2s[e];
                const double av = co < c2 && (int)c2s[e] == kq ? gv : 0.0;
                acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[rt], 0, 0, 0);
            }
    }
#pragma unroll
    for (int rt = 0; rt < GC2_MAX_RT2; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) wred[wave][rt][r * 64 + l] = acc[rt][r];
    __syncthreads();
    {
        const int r = tid >> 6, rowl = kq + 4 * r;
        for (int rt = 0; rt < nrt; ++rt) {
            const double v = ((wred[0][rt][tid] + wred[1][rt][tid]) + wred[2][rt][tid]) + wred[3][rt][tid];
            pout[((size_t)tile * 16 * nrt + 16 * rt + rowl) * 16 + s16] = v;
        }
    }
}

// A D1 item: band `band` of pooled-1 rows for one position: dA1, then the
// band's share of Gw1 | Gb1
template <int K>
__device__ __forceinline__ void gc2_d1_item(const GradCnn2Args &a, const char *scr, int64_t row, int band,
                                            double *pout, char *ldsb) {
    constexpr int KK = K * K;
    const Cnn2Dims &m = a.m;
    const GradCnn2Plan &p = a.p;
    const int tid = threadIdx.x, l = tid & 63, s16 = l & 15, kq = l >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c1 = m.c1, c2 = m.c2, T1 = m.T1, T2 = m.T2, np2 = m.np2, pw1 = m.pw1, pad = m.pad;
    const int bw = p.bw, dps = p.dps, nbm = p.nbm, xw = p.xw, xps = p.xps, nrt = p.nrt1;
    const int np1 = m.ph1 * pw1;
    double *const dpb = (double *)ldsb, *const dam = dpb + c2 * dps;
    float *const w2s = (float *)(dam + 16 * nrt * nbm), *const xs = w2s + c2 * T2;
    u8 *const c1s = (u8 *)(xs + m.c_in * xps);
    const double *g2g = (const double *)scr;
    const float *A1g = (const float *)(scr + p.o_a1);
    const u8 *c1g = (const u8 *)(scr + p.o_c1), *c2g = (const u8 *)(scr + p.o_c2);
    const int y0 = GC2_BH * band;
    const int bh = m.ph1 - y0 < GC2_BH ? m.ph1 - y0 : GC2_BH, nb = bh * pw1;
    const int64_t o_w2 = (int64_t)c1 * T1 + c1;
    // conv2's weights as they lie; the band's dP2, zero outside the kept
    // positions; pool 1's codes; the input rows the band's conv1 positions read
    for (int i = tid; i < c2 * T2; i += GC2_NT) w2s[i] = (float)a.ww[o_w2 + i];
    for (int i = tid; i < c2 * dps; i += GC2_NT) {
        const int co = i / dps, r = i - co * dps, j = r / bw, q = r - j * bw;
        const int oy = y0 + pad - (K - 1) + j, ox = pad - (K - 1) + q;
        double v = 0.0;
        if (j < GC2_BH + K - 1 && oy >= 0 && oy < 2 * m.ph2 && ox >= 0 && ox < 2 * m.pw2) {
            const int e = co * np2 + (oy >> 1) * m.pw2 + (ox >> 1);
            if ((int)c2g[e] == (oy & 1) * 2 + (ox & 1)) v = g2g[e];
        }
        dpb[i] = v;
    }
    for (int i = tid; i < 16 * nrt * nbm; i += GC2_NT) {
        const int c = i / nbm, q = i - c * nbm;
        c1s[i] = c < c1 && q < nb ? c1g[c * np1 + y0 * pw1 + q] : (u8)4;  // 4: selects nothing
        dam[i] = 0.0;
    }
    {
        const float *__restrict__ img = a.X + row * ((int64_t)m.c_in * m.h * m.w);
        for (int i = tid; i < m.c_in * xps; i += GC2_NT) {
            const int ci = i / xps, r = i - ci * xps, j = r / xw, q = r - j * xw;
            const int iy = 2 * y0 - pad + j, ix = q - pad;
            const bool in = iy >= 0 && iy < m.h && ix >= 0 && ix < m.w;
            xs[i] = in ? img[(ci * m.h + iy) * m.w + ix] : 0.0f;
        }
    }
    __syncthreads();
    // ---- dA1: rows ci, columns the band's positions, k = (co, ky, kx) ascending
    {
        const int nct = (nb + 15) >> 4, nsteps = (c2 * KK + 3) >> 2;
#pragma unroll 1
        for (int item = wave; item < nrt * nct; item += GC2_NT / 64) {
            const int ct = item / nrt, rt = item - ct * nrt;
            const int q = 16 * ct + s16, qc = q < nb ? q : 0;
            const int yl = qc / pw1, x1 = qc - yl * pw1;
            const int base = (yl + K - 1) * bw + x1 + K - 1;
            const int ci = 16 * rt + s16;
            const bool aon = ci < c1;
            const float *wrow = w2s + (aon ? ci : 0) * KK;
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
            for (int st = 0; st < nsteps; ++st) {
                const int kk = 4 * st + kq;
                const bool kin = kk < c2 * KK;
                const int kc = kin ? kk : 0, co = kc / KK, tt = kc - co * KK, ky = tt / K, kx = tt - ky * K;
                const float wv = wrow[co * T2 + tt];
                const double dv = dpb[co * dps + base - ky * bw - kx];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aon && kin ? (double)wv : 0.0,
                                                           kin && q < nb ? dv : 0.0, acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = 16 * rt + kq + 4 * r;
                if (c < c1 && q < nb) {
                    const float av = A1g[c * m.ps1 + (y0 + yl + pad) * m.P1w + x1 + pad];
                    dam[c * nbm + q] = av > 0.0f ? acc[r] : (av != av ? (double)av : 0.0);
                }
            }
        }
    }
    __syncthreads();
    // ---- Gw1 | Gb1: rows c, columns (ci, ky, kx) then the bias, k = the band's
    // conv1 positions: pooled position ascending, its window one MFMA step
    {
        const int rt = wave >> 1, ct = wave & 1;
        if (rt < nrt && 16 * ct < T1 + 1) {
            const int tcol = 16 * ct + s16, tc = tcol < T1 ? tcol : T1 - 1;
            const int ci = tc / KK, tt = tc - ci * KK, ky = tt / K, kx = tt - ky * K;
            const int xoff = ci * xps + ((kq >> 1) + ky) * xw + (kq & 1) + kx;
            const int c = 16 * rt + s16;  // < 16 nrt: c1s / dam hold 4 / 0 past c1
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};
            for (int yl = 0; yl < bh; ++yl)
                for (int x1 = 0; x1 < pw1; ++x1) {
                    const int q = yl * pw1 + x1;
                    const double gv = dam[c * nbm + q];
                    const double av = (int)c1s[c * nbm + q] == kq ? gv : 0.0;
                    const float xv = xs[xoff + 2 * yl * xw + 2 * x1];
                    const double bv = tcol < T1 ? (double)xv : tcol == T1 ? 1.0 : 0.0;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
                }
#pragma unroll
            for (int r = 0; r < 4; ++r)
                pout[((size_t)band * 16 * nrt + 16 * rt + kq + 4 * r) * 32 + tcol] = acc[r];
        }
    }
}

template <int K>
__global__ __launch_bounds__(GC2_NT) void k_grad_cnn2_bwd(const GradCnn2Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double wred[4][GC2_MAX_RT2][256];
    const int nit = a.p.nw2 + a.p.nd1;
    const int64_t s = (int64_t)blockIdx.x / nit;
    const int item = (int)((int64_t)blockIdx.x - s * nit);
    char *const scr = a.scr + s * a.p.stride;
    if (item < a.p.nw2)
        gc2_w2_item<K>(a, scr, item, (double *)(scr + a.p.o_pw2), (char *)lds, wred);
    else
        gc2_d1_item<K>(a, scr, gc2_row(a, s), item - a.p.nw2, (double *)(scr + a.p.o_pd1), (char *)lds);
}

// entry i of the gradient = thread i
__global__ __launch_bounds__(GC2_NT) void k_grad_cnn2_sum(const GradCnn2Args a) {
    __shared__ double red[GRAD_TILE];
    __shared__ unsigned int s_last;
    const Cnn2Dims &m = a.m;
    const GradCnn2Plan &p = a.p;
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * GC2_NT + tid, N = a.count, F = m.F;
    const int c1 = m.c1, c2 = m.c2, T1 = m.T1, T2 = m.T2, C = m.C;
    const int64_t o_b1 = (int64_t)c1 * T1, o_w2 = o_b1 + c1, o_b2 = o_w2 + (int64_t)c2 * T2,
                  o_fw = o_b2 + c2, o_fb = o_fw + (int64_t)C * F;
    const double cd = (double)N;
    double ss = 0.0;
    if (i < m.d) {
        double tot = 0.0;
        if (i < o_w2) {  // conv1: the D1 items' parts
            const int c = i < o_b1 ? (int)(i / T1) : (int)(i - o_b1), t = i < o_b1 ? (int)(i - (int64_t)c * T1) : T1;
            for (int64_t s = 0; s < N; ++s) {
                const double *pd = (const double *)(a.scr + s * p.stride + p.o_pd1);
                for (int b = 0; b < p.nd1; ++b) tot = tot + pd[((size_t)b * 16 * p.nrt1 + c) * 32 + t];
            }
        } else if (i < o_fw) {  // conv2: the one W2 item that holds the column
            const int64_t j = i - o_w2;
            const int co = i < o_b2 ? (int)(j / T2) : (int)(i - o_b2), t = i < o_b2 ? (int)(j - (int64_t)co * T2) : T2;
            const size_t e = ((size_t)(t >> 4) * 16 * p.nrt2 + co) * 16 + (t & 15);
            for (int64_t s = 0; s < N; ++s) tot = tot + ((const double *)(a.scr + s * p.stride + p.o_pw2))[e];
        } else if (i < o_fb) {  // GW: the chain over the positions
            const int64_t j = i - o_fw;
            const int c = (int)(j / F);
            const int64_t f = j - (int64_t)c * F;
            for (int64_t s = 0; s < N; ++s) {
                const char *scr = a.scr + s * p.stride;
                tot = __builtin_fma(((const double *)(scr + p.o_r))[c], (double)((const float *)(scr + p.o_a2))[f], tot);
            }
        } else {
            const int c = (int)(i - o_fb);
            for (int64_t s = 0; s < N; ++s)
                tot = __builtin_fma(((const double *)(a.scr + s * p.stride + p.o_r))[c], 1.0, tot);
        }
        const double g = tot / cd;
        a.G[i] = g;
        ss = g * g;
    }
    ss = grad_tree(red, ss);
    if (tid == 0) a.ssq[blockIdx.x] = ss;
    if (!grad_last_out(a.cnt, gridDim.x, &s_last)) return;
    // the last workgroup out: the workgroups' sums of squares, workgroup w in
    // lane (w mod 256)'s sum, then the tree; the loss by bk_grad_softmax's rule
    ss = 0.0;
    for (unsigned int w = tid; w < gridDim.x; w += GC2_NT) ss = ss + a.ssq[w];
    ss = grad_tree(red, ss);
    if (tid < 64) {
        double loss = 0.0;
        for (int64_t g0 = 0; g0 < N; g0 += 64) {
            const int64_t q = g0 + tid;
            double ls = q < N ? ((const double *)(a.scr + q * p.stride + p.o_r))[16] : 0.0;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) ls = ls + __shfl_xor(ls, off);  // a fixed tree
            loss = g0 == 0 ? ls : loss + ls;
        }
        if (tid == 0) {
            const double norm = __builtin_sqrt(ss);
            a.scal[1] = norm;
            a.scal[2] = a.max_norm / (norm + 1e-6);
            a.out->loss = loss / cd;
            a.out->norm = norm;
        }
    }
}

// entries 2 i, 2 i + 1 of thread i.  vec: every pointer is 16-byte aligned
__global__ __launch_bounds__(GC2_NT) void k_grad_cnn2_tail(const GradCnn2Args a, int vec) {
    const int64_t d = a.m.d;
    const int64_t i = ((int64_t)blockIdx.x * GC2_NT + threadIdx.x) * 2;
    if (i >= d) return;
    const double coef = a.scal[2];
    const bool clip = !(coef >= 1.0);  // below 1, or a NaN norm: every entry NaN
    if (vec && i + 1 < d) {
        d2 g = *(const d2 *)(a.G + i);
        if (clip) g = g * coef;
        d2 dl = -g;
        if (a.noise) dl = dl + *(const d2 *)(a.noise + i);
        *(d2 *)(a.delta + i) = dl;
        if (a.q) {
            ll2 q;
            q.x = grad_i64(dl.x * a.scale);
            q.y = grad_i64(dl.y * a.scale);
            *(ll2 *)(a.q + i) = q;
        }
        return;
    }
    for (int64_t e = i; e < d && e < i + 2; ++e) {
        double g = a.G[e];
        if (clip) g = g * coef;
        double dl = -g;
        if (a.noise) dl = dl + a.noise[e];
        a.delta[e] = dl;
        if (a.q) a.q[e] = grad_i64(dl * a.scale);
    }
}

static bool gc2_args_ok(const GradCnn2Args &a) {
    const Cnn2Dims &m = a.m;
    GradCnn2Plan p;
    return a.count >= 1 && a.count <= GRAD_CNN2_MAX_BATCH && a.nn >= 1 && m.k >= 1 && m.k <= 3 &&
           m.c_in >= 1 && m.c_in <= 3 && m.c1 >= 1 && m.c1 <= 16 * GC2_MAX_RT1 && m.c2 >= 1 &&
           m.c2 <= 16 * GC2_MAX_RT2 && m.C >= 2 && m.C <= 16 && grad_cnn2_plan(m, &p) &&
           p.lds_fwd == a.p.lds_fwd && p.lds_bwd == a.p.lds_bwd && p.stride == a.p.stride &&
           p.nw2 == a.p.nw2 && p.nd1 == a.p.nd1 && p.npl == a.p.npl && p.dps == a.p.dps && a.scr && a.G &&
           a.ssq && a.scal && a.cnt && a.out && a.delta;
}

template <int K>
static hipError_t launch_fb_k(const GradCnn2Args &a, bool bwd, hipStream_t st) {
    // per device, so asked on every launch: the LDS exceeds the default 64 KiB
    const void *f = bwd ? (const void *)k_grad_cnn2_bwd<K> : (const void *)k_grad_cnn2_fwd<K>;
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, GC2_LDS);
    if (e != hipSuccess) return e;
    if (bwd)
        hipLaunchKernelGGL(k_grad_cnn2_bwd<K>, dim3((unsigned)(a.count * (a.p.nw2 + a.p.nd1))), dim3(GC2_NT),
                           (size_t)a.p.lds_bwd, st, a);
    else
        hipLaunchKernelGGL(k_grad_cnn2_fwd<K>, dim3((unsigned)a.count), dim3(GC2_NT), (size_t)a.p.lds_fwd, st, a);
    return hipGetLastError();
}

static hipError_t launch_fb(const GradCnn2Args &a, bool bwd, hipStream_t st) {
    if (!gc2_args_ok(a)) return hipErrorInvalidConfiguration;
    switch (a.m.k) {
    case 1: return launch_fb_k<1>(a, bwd, st);
    case 2: return launch_fb_k<2>(a, bwd, st);
    default: return launch_fb_k<3>(a, bwd, st);
    }
}

hipError_t launch_grad_cnn2_fwd(const GradCnn2Args &a, hipStream_t st) { return launch_fb(a, false, st); }
hipError_t launch_grad_cnn2_bwd(const GradCnn2Args &a, hipStream_t st) { return launch_fb(a, true, st); }

hipError_t launch_grad_cnn2_sum(const GradCnn2Args &a, hipStream_t st) {
    if (!gc2_args_ok(a)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_grad_cnn2_sum, dim3((unsigned)((a.m.d + GC2_NT - 1) / GC2_NT)), dim3(GC2_NT), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_grad_cnn2_tail(const GradCnn2Args &a, hipStream_t st) {
    if (!gc2_args_ok(a)) return hipErrorInvalidConfiguration;
    const uintptr_t bits = (uintptr_t)a.G | (uintptr_t)a.noise | (uintptr_t)a.delta | (uintptr_t)a.q;
    const int64_t threads = (a.m.d + 1) / 2;
    hipLaunchKernelGGL(k_grad_cnn2_tail, dim3((unsigned)((threads + GC2_NT - 1) / GC2_NT)), dim3(GC2_NT), 0, st,
                       a, (bits & 15) == 0 ? 1 : 0);
    return hipGetLastError();
}

}  // namespace bk
