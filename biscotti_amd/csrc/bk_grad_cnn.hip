// bk_grad_cnn.hip -- the gradient step of the one-layer CNN (bk.h bk_grad_cnn,
// DESIGN.md §5z), gfx950: the backward half of the model k_cnn (bk_cnn.hip)
// scores, on the peer's resident shard.  Client.getGrad (ML/Pytorch/
// client.py:38-65) on MNISTCNNModel, negated (client_obj.py:73-77), and the
// quantisation behind it (updateFloatToInt).
//
// The unit of work is ONE OUTPUT ROW y with all c_out channels: the grid is oh
// workgroups of four waves, and a workgroup walks the batch in tiles of ts <= 16
// positions (grad_cnn_tiling).  Under that split every product of the step is a
// v_mfma_f64_16x16x4_f64 with 16 rows:
//
//   k_grad_cnn_fwd   the k input rows that row y reads go into LDS as zero-padded
//                    fp32 rows, gathered through the batch's row numbers; the
//                    row's c_out ow ts activations are k_cnn's tap chains, bit for
//                    bit, written to LDS.  Per channel one MFMA chain over x
//                    (classes x positions, the feature as the MFMA's k), the
//                    channels dealt over the waves; the chains are added over the
//                    channels in order and the row's part of the logits goes to
//                    Rp[y].  The last workgroup out adds the parts in y order and
//                    takes k_grad_softmax_fwd's softmax, residual and loss
//   k_grad_cnn_bwd   recomputes the row's activations (they never leave LDS), then
//                    per block of 16 features (a wave takes every fourth):
//                    (a) GW  = r^T a, the batch position as k, added to the running
//                        sum the workgroup owns in G (its entries belong to it alone);
//                    (c) dA  = r W, the class as k, the fc weights read from L2
//                        before (a)'s MFMAs are issued; masked by the activation
//                        into g in LDS;
//                    then (d) the conv gradient, channels x taps with (position, x)
//                    as k: the im2col view of the staged rows, a spare column held
//                    at 1 for the conv bias, one wave per block of 16 columns.
//                    The workgroup divides its fc entries by the count and sums
//                    their squares; the last workgroup out adds the conv parts in
//                    y order, takes the fc bias from R, and writes norm and coef
//   k_grad_cnn_tail  grid-wide over the d entries: clip, negate, add the noise,
//                    quantise, store; 16-byte accesses where every pointer allows
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

constexpr int GC_TS = 16;                // positions per tile: the MFMA's rows / columns
constexpr size_t GC_LDS = 128 * 1024;    // the dynamic LDS budget of the backward
constexpr int GC_MAX_K = 5, GC_MAX_CO = 16, GC_MAX_OW = 68;

// bk.h's tiling: the largest ts <= 16 for which the backward's rows (fp32),
// activations (fp32) and g (fp64) fit GC_LDS
GradCnnTiling grad_cnn_tiling(const CnnDims &m) {
    GradCnnTiling t = {};
    const int rows = m.k * m.pw;
    t.rs = rows + ((4 - rows % 64) + 64) % 64;  // 4 mod 64 words: 16 positions x 4 features, 64 banks
    t.J = m.co * m.ow;
    int ts = GC_TS;
    while (ts > 1 && (size_t)4 * ts * t.rs + (size_t)12 * t.J * (ts + 1) > GC_LDS) --ts;
    t.ts = ts;
    t.as = ts + 1;  // odd: a feature block's 16 rows fall into distinct banks
    t.lds_fwd = sizeof(float) * ((size_t)t.J * t.as + (size_t)ts * t.rs);
    t.lds_bwd = t.lds_fwd + sizeof(double) * (size_t)t.J * t.as;
    return t;
}

// A tile of the batch for output row y: the rows' numbers, the k input rows of
// every position (zero-padded; a missing position is all zeros) and the row's
// activations act[j as + s], j = ch ow + x (0 for a missing position).  The tap
// chain is k_cnn's.  Ends behind a barrier
template <int K>
__device__ __forceinline__ void gc_tile(const GradCnnArgs &a, int y, int64_t p0, int cnt, float *xr,
                                        float *act, const double *cw, const double *cb,
                                        int64_t *rown) {
    const CnnDims &m = a.m;
    const int tid = threadIdx.x;
    const int ts = a.t.ts, as = a.t.as, rs = a.t.rs, J = a.t.J;
    __syncthreads();  // the previous tile has been consumed
    if (tid < GC_TS) {
        int64_t p = p0 + tid;
        p = p < a.count ? p : a.count - 1;
        int64_t row = a.rows ? a.rows[p] : p;
        if (row < 0 || row >= a.nn) row = 0;  // the host entry has refused it; never out of range
        rown[tid] = row;
    }
    __syncthreads();
    const float *__restrict__ X = a.X;
    const int kp = K * m.pw, hw = m.h * m.w;
    for (int i = tid; i < ts * kp; i += 256) {
        const int s = i / kp, r = i - s * kp, ky = r / m.pw, xx = r - ky * m.pw;
        const int iy = y + ky - m.pad, ix = xx - m.pad;
        const bool in = s < cnt && iy >= 0 && iy < m.h && ix >= 0 && ix < m.w;
        xr[s * rs + r] = in ? X[rown[s] * hw + iy * m.w + ix] : 0.0f;
    }
    __syncthreads();
    const int s = tid & 15;
    for (int j = tid >> 4; j < J; j += 16) {
        if (s >= ts) continue;
        const int ch = j / m.ow, x = j - ch * m.ow;
        const float *px = xr + s * rs + x;
        const double *pw = cw + ch * (K * K);
        double acc = 0.0;
#pragma unroll
        for (int ky = 0; ky < K; ++ky)
#pragma unroll
            for (int kx = 0; kx < K; ++kx)
                acc = __builtin_fma((double)px[ky * m.pw + kx], pw[ky * K + kx], acc);
        const float pre = (float)(acc + cb[ch]);
        const float av = pre < 0.0f ? 0.0f : pre;  // a NaN stays
        act[j * as + s] = s < cnt ? av : 0.0f;
    }
    __syncthreads();
}

// the conv weights and biases as doubles of their fp32 values
template <int K>
__device__ __forceinline__ void gc_conv_model(const GradCnnArgs &a, double *cw, double *cb) {
    const int tid = threadIdx.x, co = a.m.co;
    for (int i = tid; i < co * K * K; i += 256) cw[i] = (double)(float)a.ww[i];
    if (tid < GC_MAX_CO) cb[tid] = tid < co ? (double)(float)a.ww[co * K * K + tid] : 0.0;
}

template <int K>
__global__ __launch_bounds__(256) void k_grad_cnn_fwd(const GradCnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double Sb[GC_MAX_CO][GC_TS][17];  // the segment chains [ch][s][c]
    __shared__ double cw[GC_MAX_CO * K * K], cb[GC_MAX_CO], fb[16];
    __shared__ double lt[64][17];
    __shared__ int64_t rown[GC_TS];
    __shared__ unsigned int s_last;
    const CnnDims &m = a.m;
    const int tid = threadIdx.x, l = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int y = (int)blockIdx.x;
    const int C = m.C, co = m.co, ow = m.ow, oh = m.oh;
    const int ts = a.t.ts, as = a.t.as, J = a.t.J;
    const int64_t F = m.F, N = a.count;
    const int64_t o_fw = (int64_t)co * K * K + co, o_fb = o_fw + (int64_t)C * F;
    const double *__restrict__ ww = a.ww;
    float *act = lds, *xr = lds + J * as;
    gc_conv_model<K>(a, cw, cb);
    if (tid >= 64 && tid < 80) fb[tid - 64] = tid - 64 < C ? (double)(float)ww[o_fb + tid - 64] : 0.0;
    const int l15 = l & 15, kq = l >> 4;
    const int tiles = (int)((N + ts - 1) / ts);
    for (int tl = 0; tl < tiles; ++tl) {
        const int64_t p0 = (int64_t)tl * ts;
        const int cnt = (int)(N - p0 < ts ? N - p0 : ts);
        gc_tile<K>(a, y, p0, cnt, xr, act, cw, cb, rown);
        // the segment chains: classes x positions, x as the MFMA's k
        for (int ch = wave; ch < co; ch += 4) {
            const int64_t kb = o_fw + (int64_t)(l15 < C ? l15 : 0) * F + (int64_t)ch * oh * ow +
                               (int64_t)y * ow;
            double wa[GC_MAX_OW / 4];
#pragma unroll
            for (int st = 0; st < GC_MAX_OW / 4; ++st) {
                const int x = 4 * st + kq;
                const double w = ww[kb + (x < ow ? x : ow - 1)];
                wa[st] = l15 < C && x < ow ? (double)(float)w : 0.0;
            }
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};
            const float *pa = act + ch * ow * as + (l15 < ts ? l15 : 0);
#pragma unroll
            for (int st = 0; st < GC_MAX_OW / 4; ++st) {
                if (4 * st < ow) {
                    const int x = 4 * st + kq;
                    const float b = pa[(x < ow ? x : ow - 1) * as];
                    const double bv = x < ow && l15 < ts ? (double)b : 0.0;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[st], bv, acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) Sb[ch][l15][kq + 4 * r] = acc[r];
        }
        __syncthreads();
        {
            const int s = tid >> 4, c = tid & 15;
            double sum = 0.0;
            for (int ch = 0; ch < co; ++ch) sum = sum + Sb[ch][s][c];
            if (s < cnt) a.Rp[((int64_t)y * N + p0 + s) * 16 + c] = sum;
        }
    }
    if (!grad_last_out(a.cnt, gridDim.x, &s_last)) return;
    // the last workgroup out: the logits (y ascending, then the bias), then
    // k_grad_softmax_fwd's rule on groups of 64 positions, lane s of wave 0
    // taking position s
    double loss = 0.0;
    for (int64_t g0 = 0; g0 < N; g0 += 64) {
        __syncthreads();  // lt's previous use is over
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int sl = 16 * u + (tid >> 4), c = tid & 15;
            const int64_t p = g0 + sl;
            double v = 0.0;
            if (p < N) {
                for (int yy = 0; yy < oh; ++yy) v = v + a.Rp[((int64_t)yy * N + p) * 16 + c];
                v = v + fb[c];
            }
            lt[sl][c] = v;
        }
        __syncthreads();
        if (wave == 0) {
            const int64_t p = g0 + l;
            const bool valid = p < N;
            const int64_t pc = valid ? p : N - 1;
            int64_t row = a.rows ? a.rows[pc] : pc;
            if (row < 0 || row >= a.nn) row = 0;
            int yy = a.y[row];
            yy = yy < 0 || yy >= C ? 0 : yy;
            const double *lg = lt[l];
            double mx = lg[0];
            for (int c = 1; c < C; ++c) {
                const double v = lg[c];
                mx = v > mx ? v : mx;
            }
            double e[16], sum = 0.0;
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                e[c] = c < C ? exp(lg[c] - mx) : 0.0;
                if (c < C) sum = sum + e[c];
            }
            if (valid) {
                double *Rq = a.R + p * 16;
#pragma unroll
                for (int c = 0; c < 16; ++c) Rq[c] = c < C ? e[c] / sum - (c == yy ? 1.0 : 0.0) : 0.0;
            }
            double ls = valid ? log(sum) + mx - lg[yy] : 0.0;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) ls = ls + __shfl_xor(ls, off);  // a fixed tree
            loss = g0 == 0 ? ls : loss + ls;
        }
    }
    if (tid == 0) a.scal[0] = loss;
}

template <int K>
__global__ __launch_bounds__(256) void k_grad_cnn_bwd(const GradCnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double cw[GC_MAX_CO * K * K], cb[GC_MAX_CO];
    __shared__ double rsm[GC_TS][17];  // the tile's residuals r[s][c]
    __shared__ double red[GRAD_TILE];
    __shared__ int64_t rown[GC_TS];
    __shared__ unsigned int s_last;
    constexpr int T = K * K + 1;  // the taps, then the conv bias
    const CnnDims &m = a.m;
    const int tid = threadIdx.x, l = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int y = (int)blockIdx.x;
    const int C = m.C, co = m.co, ow = m.ow, oh = m.oh, pw = m.pw;
    const int ts = a.t.ts, as = a.t.as, rs = a.t.rs, J = a.t.J;
    const int64_t F = m.F, N = a.count;
    const int64_t o_fw = (int64_t)co * K * K + co, o_fb = o_fw + (int64_t)C * F;
    const double *__restrict__ ww = a.ww;
    double *__restrict__ G = a.G;
    double *gbuf = (double *)lds;  // g[j as + s]
    float *act = lds + 2 * J * as, *xr = act + J * as;
    gc_conv_model<K>(a, cw, cb);
    const int l15 = l & 15, kq = l >> 4;
    const int tiles = (int)((N + ts - 1) / ts);
    const int nfb = (J + 15) >> 4;
    for (int tl = 0; tl < tiles; ++tl) {
        const int64_t p0 = (int64_t)tl * ts;
        const int cnt = (int)(N - p0 < ts ? N - p0 : ts);
        gc_tile<K>(a, y, p0, cnt, xr, act, cw, cb, rown);
        {
            const int s = tid >> 4, c = tid & 15;
            rsm[s][c] = s < cnt ? a.R[(p0 + s) * 16 + c] : 0.0;
        }
        __syncthreads();
        for (int fbk = wave; fbk < nfb; fbk += 4) {
            const int j = 16 * fbk + l15;
            const bool jin = j < J;
            const int jc = jin ? j : J - 1;
            const int ch = jc / ow, x = jc - ch * ow;
            const int64_t kf = (int64_t)ch * oh * ow + (int64_t)y * ow + x;
            // the fc weights of the block: class 4 st + kq, feature l15
            double wv[4];
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const int c = 4 * st + kq;
                const double w = ww[o_fw + (int64_t)(c < C ? c : 0) * F + kf];
                wv[st] = jin && c < C ? (double)(float)w : 0.0;
            }
            // (a) GW: A[c][s] = r, B[s][f] = a
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const int s = 4 * st + kq;
                const float b = act[jc * as + (s < ts ? s : 0)];
                const double bv = jin && s < ts ? (double)b : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(rsm[s][l15], bv, acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = kq + 4 * r;
                if (jin && c < C) {
                    const int64_t e = o_fw + (int64_t)c * F + kf;
                    G[e] = tl == 0 ? acc[r] : G[e] + acc[r];
                }
            }
            // (c) dA: A[s][c] = r, B[c][f] = W; masked into g
            d4 da = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int st = 0; st < 4; ++st)
                da = __builtin_amdgcn_mfma_f64_16x16x4f64(rsm[l15][4 * st + kq], wv[st], da, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int s = kq + 4 * r;
                if (jin && s < ts) {
                    const float av = act[jc * as + s];
                    gbuf[jc * as + s] = av > 0.0f ? da[r] : (av != av ? (double)av : 0.0);
                }
            }
        }
        __syncthreads();
        // (d) the conv gradient: A[ch][(s, x)] = g, B[(s, x)][tap] = xpad; wave
        // w takes the columns 16 w ..
        if (wave < (T + 15) / 16) {
            const int tcol = 16 * wave + l15;
            const int tc = tcol < K * K ? tcol : 0, ky = tc / K, kx = tc - ky * K;
            const int chl = l15 < co ? l15 : 0;
            const int nk = cnt * ow, steps = (nk + 3) >> 2;
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};
            for (int st = 0; st < steps; ++st) {
                const int kk = 4 * st + kq;
                const bool ok = kk < nk;
                const int kc = ok ? kk : 0, s = kc / ow, x = kc - s * ow;
                const double gv = gbuf[(chl * ow + x) * as + s];
                const float xv = xr[s * rs + ky * pw + x + kx];
                const double av = ok && l15 < co ? gv : 0.0;
                const double bv = !ok ? 0.0 : tcol < K * K ? (double)xv : tcol == K * K ? 1.0 : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ch = kq + 4 * r;
                if (ch < co && tcol < T)
                    a.Tp[(((int64_t)tl * oh + y) * co + ch) * T + tcol] = acc[r];
            }
        }
    }
    // the fc entries of row y are this workgroup's alone: divided by the count,
    // their squares in lane (entry mod 256)'s sum, entry = c J + j ascending
    __syncthreads();
    const double cd = (double)N;
    double ss = 0.0;
    for (int el = tid; el < C * J; el += GRAD_TILE) {
        const int c = el / J, j = el - c * J, ch = j / ow, x = j - ch * ow;
        const int64_t e = o_fw + (int64_t)c * F + (int64_t)ch * oh * ow + (int64_t)y * ow + x;
        const double g = G[e] / cd;
        G[e] = g;
        ss = ss + g * g;
    }
    ss = grad_tree(red, ss);
    if (tid == 0) a.ssq[y] = ss;
    if (!grad_last_out(a.cnt, gridDim.x, &s_last)) return;
    // the last workgroup out: the conv weights, the conv biases and the fc
    // biases, entry i of that list in lane (i mod 256)'s sum
    const int ncw = co * K * K, nconv = ncw + co;
    ss = 0.0;
    for (int i = tid; i < nconv + C; i += GRAD_TILE) {
        double tot = 0.0;
        if (i < nconv) {
            const int ch = i < ncw ? i / (K * K) : i - ncw, t = i < ncw ? i - ch * (K * K) : K * K;
            for (int tl = 0; tl < tiles; ++tl) {
                double v = 0.0;
                for (int yy = 0; yy < oh; ++yy) v = v + a.Tp[(((int64_t)tl * oh + yy) * co + ch) * T + t];
                tot = tl == 0 ? v : tot + v;
            }
        } else {
            const int c = i - nconv;
            for (int tl = 0; tl < tiles; ++tl) {
                const int64_t p0 = (int64_t)tl * ts;
                const int cnt = (int)(N - p0 < ts ? N - p0 : ts);
                double v = 0.0;
                for (int s = 0; s < cnt; ++s) v = __builtin_fma(a.R[(p0 + s) * 16 + c], 1.0, v);
                tot = tl == 0 ? v : tot + v;
            }
        }
        const double g = tot / cd;
        G[i < nconv ? (int64_t)i : o_fb + (i - nconv)] = g;
        ss = ss + g * g;
    }
    ss = grad_tree(red, ss);
    if (tid == 0) {
        double s2 = a.ssq[0];
        for (int yy = 1; yy < oh; ++yy) s2 = s2 + a.ssq[yy];
        s2 = s2 + ss;
        const double norm = __builtin_sqrt(s2);
        a.scal[1] = norm;
        a.scal[2] = a.max_norm / (norm + 1e-6);
        a.out->loss = a.scal[0] / cd;
        a.out->norm = norm;
    }
}

// entries 2 i, 2 i + 1 of thread i.  vec: every pointer is 16-byte aligned
__global__ __launch_bounds__(256) void k_grad_cnn_tail(const GradCnnArgs a, int vec) {
    const int64_t d = a.m.d;
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
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

static bool gc_args_ok(const GradCnnArgs &a) {
    const CnnDims &m = a.m;
    const GradCnnTiling t = grad_cnn_tiling(m);
    return a.count >= 1 && a.count <= GRAD_CNN_MAX_BATCH && a.nn >= 1 && m.k >= 1 && m.k <= GC_MAX_K &&
           m.co >= 1 && m.co <= GC_MAX_CO && m.C >= 2 && m.C <= 16 && m.ow >= 1 && m.ow <= GC_MAX_OW &&
           m.oh >= 1 && t.ts == a.t.ts && t.as == a.t.as && t.rs == a.t.rs && t.J == a.t.J &&
           t.lds_bwd == a.t.lds_bwd && t.lds_fwd == a.t.lds_fwd && t.lds_bwd <= GC_LDS;
}

template <int K>
static hipError_t launch_fwd_k(const GradCnnArgs &a, hipStream_t st) {
    // per device, so asked on every launch: the LDS may exceed the default 64 KiB
    const hipError_t e = hipFuncSetAttribute((const void *)k_grad_cnn_fwd<K>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.t.lds_fwd);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_grad_cnn_fwd<K>, dim3((unsigned)a.m.oh), dim3(256), a.t.lds_fwd, st, a);
    return hipGetLastError();
}

template <int K>
static hipError_t launch_bwd_k(const GradCnnArgs &a, hipStream_t st) {
    const hipError_t e = hipFuncSetAttribute((const void *)k_grad_cnn_bwd<K>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.t.lds_bwd);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_grad_cnn_bwd<K>, dim3((unsigned)a.m.oh), dim3(256), a.t.lds_bwd, st, a);
    return hipGetLastError();
}

hipError_t launch_grad_cnn_fwd(const GradCnnArgs &a, hipStream_t st) {
    if (!gc_args_ok(a)) return hipErrorInvalidConfiguration;
    switch (a.m.k) {
    case 1: return launch_fwd_k<1>(a, st);
    case 2: return launch_fwd_k<2>(a, st);
    case 3: return launch_fwd_k<3>(a, st);
    case 4: return launch_fwd_k<4>(a, st);
    default: return launch_fwd_k<5>(a, st);
    }
}

hipError_t launch_grad_cnn_bwd(const GradCnnArgs &a, hipStream_t st) {
    if (!gc_args_ok(a)) return hipErrorInvalidConfiguration;
    switch (a.m.k) {
    case 1: return launch_bwd_k<1>(a, st);
    case 2: return launch_bwd_k<2>(a, st);
    case 3: return launch_bwd_k<3>(a, st);
    case 4: return launch_bwd_k<4>(a, st);
    default: return launch_bwd_k<5>(a, st);
    }
}

hipError_t launch_grad_cnn_tail(const GradCnnArgs &a, hipStream_t st) {
    if (!gc_args_ok(a)) return hipErrorInvalidConfiguration;
    const uintptr_t bits = (uintptr_t)a.G | (uintptr_t)a.noise | (uintptr_t)a.delta | (uintptr_t)a.q;
    const int64_t threads = (a.m.d + 1) / 2;
    hipLaunchKernelGGL(k_grad_cnn_tail, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, a,
                       (bits & 15) == 0 ? 1 : 0);
    return hipGetLastError();
}

}  // namespace bk
