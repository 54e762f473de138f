// bk_grad.hip -- a peer's gradient step, gfx950: the backward
// half of the models bk_eval.hip scores, on the peer's resident shard.
//
// computeUpdate -> oneGradientStep (DistSys/honest.go:165-200, 284-324) calls
//     logistic  privateFun / funObj      (ML/code/logistic_model.py:92-140)
//     softmax   Client.getGrad, negated  (ML/Pytorch/client.py:38-65,
//                                         client_obj.py:73-77)
// and quantises the delta at once (updateFloatToInt, honest.go:183).
//
//   k_grad_logistic  a workgroup takes one tile of 256 batch positions, its rows
//                    gathered through the caller's row numbers.  Thread t takes
//                    position t: z as k_eval_sign's fp64 FMA chain over k
//                    ascending from +0.0 (d <= 32: the row straight into
//                    registers and on into LDS; beyond: through LDS in chunks of
//                    32 features), res = -y / (1 + e^{y z}) and the loss part.
//                    Then thread j takes feature j: the tile's FMA chain over
//                    its positions ascending from +0.0 of X[r_i][j] res_i (rows
//                    from LDS at d <= 32, else from L2, a row's features across
//                    the lanes).  One tile: the workgroup writes the tail
//                    itself.  More: the tile sums go to a buffer and the last
//                    workgroup out adds them in tile order
//   k_grad_softmax_fwd  k_eval_logits' staging and MFMAs on the gathered rows,
//                    64 positions a workgroup; the logits stay fp64.  Lane s of
//                    wave 0 takes position s: softmax over c ascending, the
//                    residual row R[s][0..16) (zero past C) and the loss part
//   k_grad_softmax_bwd  R^T X on v_mfma_f64_16x16x4_f64, the batch position as
//                    the MFMA's k: a wave takes 16 features (the bias is the
//                    feature d_in, its x = 1) and all 16 class rows, one chain
//                    from +0.0 per tile of 256 positions, the tiles' results
//                    added in tile order.  The last workgroup out divides by
//                    the count, sums the squares, clips, negates, adds the
//                    noise, quantises and stores
//
// Nobody waits for anybody: every hand-off is the last arriver's (plain stores,
// every wave's vmcnt(0), a barrier, lane 0's agent release and counter add; the
// workgroup whose add came last acquires and reads).  Every sum has one fixed
// order, whatever the grid or the timing.  Built with -ffp-contract=off: only
// the chains are FMAs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bk_ctx.h"

namespace bk {

typedef double d4 __attribute__((ext_vector_type(4)));

// Go (amd64) int64(float64), k_qsum's rule: truncation; NaN and values outside
// [-2^63, 2^63) give 0x8000000000000000
__device__ __forceinline__ int64_t grad_i64(double y) {
    if (y >= -9223372036854775808.0 && y < 9223372036854775808.0) return (int64_t)y;
    return INT64_MIN;
}

// Behind a workgroup's plain stores of handed-off data: true, in every thread,
// for the workgroup that left last of `total`; its loads then see every other
// workgroup's stores.  It puts the counter back to zero for the next launch
__device__ inline bool grad_last_out(unsigned int *cnt, unsigned int total, unsigned int *s_last) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const bool last = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT) == total - 1u;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        *s_last = last ? 1u : 0u;
    }
    __syncthreads();
    return *s_last != 0u;
}

// red[0] = the 256 values' sum by the fixed tree (strides 128, 64, .. 1)
__device__ inline double grad_tree(double *red, double v) {
    const int tid = threadIdx.x;
    __syncthreads();  // red's previous use is over
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = GRAD_TILE / 2; s >= 1; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// delta_j (and q_j) from the batch's S_j
__device__ __forceinline__ void grad_logistic_store(const GradLogistic &a, int64_t j, double S) {
    const double g = S / a.batch + a.lammy * a.ww[j];
    double dl = -a.alpha * g;
    if (a.noise) dl = dl + a.noise[j];
    a.delta[j] = dl;
    if (a.q) a.q[j] = grad_i64(dl * a.scale);
}

constexpr int GL_KC = 32;

template <bool REG>
__global__ __launch_bounds__(256) void k_grad_logistic(const GradLogistic a) {
    __shared__ double xs[GRAD_TILE][GL_KC + 1];
    __shared__ double wsm[GL_KC];
    __shared__ double res[GRAD_TILE], red[GRAD_TILE];
    __shared__ int64_t rown[GRAD_TILE];
    __shared__ unsigned int s_last;
    const int tid = threadIdx.x;
    const int64_t d = a.d;
    const double *__restrict__ X = a.X;
    const int64_t p0 = (int64_t)blockIdx.x * GRAD_TILE;
    const int cnt = (int)(a.count - p0 < GRAD_TILE ? a.count - p0 : GRAD_TILE);
    {
        int64_t p = p0 + tid;
        p = p < a.count ? p : a.count - 1;
        rown[tid] = a.rows ? a.rows[p] : p;
    }
    __syncthreads();
    const int64_t r = rown[tid];
    double acc = 0.0;
    if (REG) {  // d <= 32: clamped loads, all in flight, then the chain
        const double *xr = X + r * d;
        double x[GL_KC];
#pragma unroll
        for (int k = 0; k < GL_KC; ++k) x[k] = xr[k < d ? k : d - 1];
#pragma unroll
        for (int k = 0; k < GL_KC; ++k) {
            const double w = a.ww[k < d ? k : d - 1];
            acc = k < d ? __builtin_fma(x[k], w, acc) : acc;
        }
#pragma unroll
        for (int k = 0; k < GL_KC; ++k) xs[tid][k] = x[k];
    } else {
        // k_eval_sign's staging: thread t moves feature t & 31 of positions
        // (t >> 5) + 8 u, the next chunk's loads in flight under this chain
        const int xk = tid & 31, xr = tid >> 5;
        double xv[GL_KC], wv = 0.0;
        auto load = [&](int64_t k0) {
            int64_t k = k0 + xk;
            k = k < d ? k : d - 1;
#pragma unroll
            for (int u = 0; u < GL_KC; ++u) xv[u] = X[rown[xr + 8 * u] * d + k];
            if (xr == 0) wv = a.ww[k];
        };
        load(0);
        for (int64_t k0 = 0; k0 < d; k0 += GL_KC) {
            __syncthreads();  // the previous chunk has been consumed
#pragma unroll
            for (int u = 0; u < GL_KC; ++u) xs[xr + 8 * u][xk] = xv[u];
            if (xr == 0) wsm[xk] = wv;
            __syncthreads();
            if (k0 + GL_KC < d) load(k0 + GL_KC);
            const int kn = (int)(d - k0 < GL_KC ? d - k0 : GL_KC);
            for (int kk = 0; kk < kn; ++kk) acc = __builtin_fma(xs[tid][kk], wsm[kk], acc);
        }
    }
    // res = -y / exp(logaddexp(0, t)) = -y / (1 + e^t): t -> +inf gives -+0,
    // t -> -inf gives -y; the loss part logaddexp(0, -t)
    const double y = a.y[r];
    const double t = y * acc;
    const double rs = -y / (1.0 + exp(t));
    const double mt = -t;
    const double lp = (mt > 0.0 ? mt : 0.0) + log1p(exp(-__builtin_fabs(t)));
    res[tid] = tid < cnt ? rs : 0.0;
    const double tile_loss = grad_tree(red, tid < cnt ? lp : 0.0);  // its barriers publish res, xs
    const bool one = gridDim.x == 1;
    for (int64_t j0 = 0; j0 < d; j0 += GRAD_TILE) {
        const int64_t j = j0 + tid;
        if (j >= d) break;
        double s = 0.0;
        if (REG) {
            for (int i = 0; i < cnt; ++i) s = __builtin_fma(xs[i][tid], res[i], s);
        } else {
            int i = 0;
            for (; i + 8 <= cnt; i += 8) {
                double v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = X[rown[i + q] * d + j];
#pragma unroll
                for (int q = 0; q < 8; ++q) s = __builtin_fma(v[q], res[i + q], s);
            }
            for (; i < cnt; ++i) s = __builtin_fma(X[rown[i] * d + j], res[i], s);
        }
        if (one)
            grad_logistic_store(a, j, s);
        else
            a.part[(int64_t)blockIdx.x * d + j] = s;
    }
    double loss = tile_loss;
    if (!one) {
        if (tid == 0) a.lossp[blockIdx.x] = tile_loss;
        if (!grad_last_out(a.cnt, gridDim.x, &s_last)) return;
        const int tiles = (int)gridDim.x;
        for (int64_t j = tid; j < d; j += GRAD_TILE) {
            double S = a.part[j];
            for (int tl = 1; tl < tiles; ++tl) S = S + a.part[(int64_t)tl * d + j];
            grad_logistic_store(a, j, S);
        }
        loss = a.lossp[0];
        for (int tl = 1; tl < tiles; ++tl) loss = loss + a.lossp[tl];
    }
    // the diagnostic's 0.5 lammy ww.ww: feature j in lane j mod 256's sum, then the tree
    double w2 = 0.0;
    for (int64_t j = tid; j < d; j += GRAD_TILE) w2 = w2 + a.ww[j] * a.ww[j];
    w2 = grad_tree(red, w2);
    if (tid == 0) {
        a.out->loss = loss + 0.5 * a.lammy * w2;
        a.out->norm = 0.0;
    }
}

// ---- softmax ------------------------------------------------------------------
// the forward: k_eval_logits' chunks of 64 features through LDS (row stride 68
// floats), per k-step of 4 one MFMA a wave (A: its 16 positions, B: the 16
// class rows, fp32 values widened: the products are exact).  D reg r of lane l
// is row (l >> 4) + 4 r, column l & 15
constexpr int GS_TS = 64, GS_KC = 64, GS_XS = 68;

__global__ __launch_bounds__(256) void k_grad_softmax_fwd(const GradSoftmax a) {
    __shared__ float xs[GS_TS][GS_XS];
    __shared__ float wsf[16][GS_XS];
    __shared__ double lt[GS_TS][17];
    __shared__ double bl[16];
    __shared__ int64_t rown[GS_TS];
    const int tid = threadIdx.x, l = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t din = a.din;
    const int C = a.C;
    const float *__restrict__ X = a.X;
    const double *__restrict__ ww = a.ww;
    const int64_t p0 = (int64_t)blockIdx.x * GS_TS;
    if (tid < GS_TS) {
        int64_t p = p0 + tid;
        p = p < a.count ? p : a.count - 1;
        rown[tid] = a.rows ? a.rows[p] : p;
    }
    if (tid < 16)  // the model's fp32 biases
        bl[tid] = tid < C ? (double)(float)ww[(int64_t)C * din + tid] : 0.0;
    __syncthreads();
    // staging: thread t moves feature t & 63 of positions / classes (t >> 6) + 4 u
    const int xk = tid & 63, xr = tid >> 6;
    float xv[16], wv[4];
    auto load = [&](int64_t k0) {  // clamped addresses, every load in flight
        const int64_t k = k0 + xk;
        const bool kin = k < din;
        const int64_t kc = kin ? k : din - 1;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const float x = X[rown[xr + 4 * u] * din + kc];
            xv[u] = kin ? x : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = xr + 4 * u;
            const double w = ww[(int64_t)(c < C ? c : C - 1) * din + kc];
            wv[u] = kin && c < C ? (float)w : 0.0f;
        }
    };
    d4 acc = d4{0.0, 0.0, 0.0, 0.0};
    const int arow = 16 * wave + (l & 15), ak = l >> 4;
    load(0);
    for (int64_t k0 = 0; k0 < din; k0 += GS_KC) {
        __syncthreads();  // the previous chunk has been consumed
#pragma unroll
        for (int u = 0; u < 16; ++u) xs[xr + 4 * u][xk] = xv[u];
#pragma unroll
        for (int u = 0; u < 4; ++u) wsf[xr + 4 * u][xk] = wv[u];
        __syncthreads();
        if (k0 + GS_KC < din) load(k0 + GS_KC);
        const int kn = (int)(din - k0 < GS_KC ? din - k0 : GS_KC);
        const int steps = (kn + 3) >> 2;  // features past d_in are zero in LDS
        for (int st = 0; st < steps; ++st) {
            const double av = (double)xs[arow][4 * st + ak];
            const double bv = (double)wsf[l & 15][4 * st + ak];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) lt[16 * wave + (l >> 4) + 4 * r][l & 15] = acc[r] + bl[l & 15];
    __syncthreads();
    if (tid >= GS_TS) return;  // wave 0: lane s takes position s (no barrier below)
    const int64_t p = p0 + l;
    const bool valid = p < a.count;
    const double *lg = lt[l];
    double m = lg[0];
    for (int c = 1; c < C; ++c) {
        const double v = lg[c];
        m = v > m ? v : m;
    }
    double e[16], sum = 0.0;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        e[c] = c < C ? exp(lg[c] - m) : 0.0;
        if (c < C) sum = sum + e[c];
    }
    const int yy = a.y[rown[l]];
    if (valid) {
        double *Rp = a.R + p * 16;
#pragma unroll
        for (int c = 0; c < 16; ++c) Rp[c] = c < C ? e[c] / sum - (c == yy ? 1.0 : 0.0) : 0.0;
    }
    double ls = valid ? log(sum) + m - lg[yy] : 0.0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ls = ls + __shfl_xor(ls, off);  // a fixed tree
    if (l == 0) a.lossp[blockIdx.x] = ls;
}

// the backward: a workgroup takes 64 features (a wave 16; feature d_in is the
// bias), every tile of 256 positions in turn.  A lane supplies A[c = l & 15]
// [k = l >> 4] = R[position][c] and B[k = l >> 4][f = l & 15] = x[position][f]
__global__ __launch_bounds__(256) void k_grad_softmax_bwd(const GradSoftmax a) {
    __shared__ int64_t rown[GRAD_TILE];
    __shared__ double red[GRAD_TILE];
    __shared__ unsigned int s_last;
    const int tid = threadIdx.x, l = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t din = a.din, count = a.count;
    const int C = a.C;
    const int64_t dm = (int64_t)C * (din + 1);
    const float *__restrict__ X = a.X;
    const double *__restrict__ R = a.R;
    const int64_t f0 = (int64_t)blockIdx.x * 64 + 16 * wave, f = f0 + (l & 15);
    const bool active = f0 <= din;  // wave-uniform
    const bool fin = f < din, fb = f == din;
    const int64_t fc = fin ? f : din - 1;
    const int kq = l >> 4, cl = l & 15;
    const int tiles = (int)((count + GRAD_TILE - 1) / GRAD_TILE);
    d4 tot = d4{0.0, 0.0, 0.0, 0.0};
    for (int tl = 0; tl < tiles; ++tl) {
        const int64_t p0 = (int64_t)tl * GRAD_TILE;
        const int cnt = (int)(count - p0 < GRAD_TILE ? count - p0 : GRAD_TILE);
        __syncthreads();  // the previous tile's rows have been consumed
        {
            int64_t p = p0 + tid;
            p = p < count ? p : count - 1;
            rown[tid] = a.rows ? a.rows[p] : p;
        }
        __syncthreads();
        if (!active) continue;
        d4 acc = d4{0.0, 0.0, 0.0, 0.0};
        const int steps = (cnt + 3) >> 2;
        for (int st = 0; st < steps; ++st) {
            const int i = 4 * st + kq;
            const bool ok = i < cnt;
            const int ic = ok ? i : cnt - 1;
            const double rv = R[(p0 + ic) * 16 + cl];
            const float xf = X[rown[ic] * din + fc];
            const double av = ok ? rv : 0.0;
            const double bv = ok ? (fin ? (double)xf : (fb ? 1.0 : 0.0)) : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
        if (tl == 0)
            tot = acc;
        else
            tot = tot + acc;
    }
    if (active && f <= din) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = kq + 4 * r;
            if (c < C) a.part[fin ? (int64_t)c * din + f : (int64_t)C * din + c] = tot[r];
        }
    }
    if (!grad_last_out(a.cnt, gridDim.x, &s_last)) return;
    // the tail.  The squares: entry e (W row-major, then the bias) in lane
    // e mod 256's sum, e ascending, then the tree
    const double cd = (double)count;
    double ss = 0.0;
    for (int64_t e = tid; e < dm; e += GRAD_TILE) {
        const double g = a.part[e] / cd;
        a.part[e] = g;
        ss = ss + g * g;
    }
    const double norm = __builtin_sqrt(grad_tree(red, ss));
    const double coef = a.max_norm / (norm + 1e-6);
    const bool clip = coef < 1.0;
    for (int64_t e = tid; e < dm; e += GRAD_TILE) {
        double g = a.part[e];
        if (clip) g = g * coef;
        double dl = -g;
        if (a.noise) dl = dl + a.noise[e];
        a.delta[e] = dl;
        if (a.q) a.q[e] = grad_i64(dl * a.scale);
    }
    if (tid == 0) {
        const int nw = (int)((count + GS_TS - 1) / GS_TS);
        double loss = a.lossp[0];
        for (int i = 1; i < nw; ++i) loss = loss + a.lossp[i];
        a.out->loss = loss / cd;
        a.out->norm = norm;
    }
}

hipError_t launch_grad_logistic(const GradLogistic &a, hipStream_t st) {
    if (a.count < 1 || a.count > GRAD_MAX_BATCH || a.d < 1 || a.d > GRAD_MAX_D)
        return hipErrorInvalidConfiguration;
    const unsigned tiles = (unsigned)((a.count + GRAD_TILE - 1) / GRAD_TILE);
    if (a.d <= GL_KC)
        hipLaunchKernelGGL(k_grad_logistic<true>, dim3(tiles), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(k_grad_logistic<false>, dim3(tiles), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_grad_softmax_fwd(const GradSoftmax &a, hipStream_t st) {
    if (a.count < 1 || a.count > GRAD_MAX_BATCH || a.din < 1 || a.din > GRAD_MAX_D || a.C < 2 ||
        a.C > 16)
        return hipErrorInvalidConfiguration;
    const unsigned wgs = (unsigned)((a.count + GS_TS - 1) / GS_TS);
    hipLaunchKernelGGL(k_grad_softmax_fwd, dim3(wgs), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_grad_softmax_bwd(const GradSoftmax &a, hipStream_t st) {
    if (a.count < 1 || a.count > GRAD_MAX_BATCH || a.din < 1 || a.din > GRAD_MAX_D || a.C < 2 ||
        a.C > 16)
        return hipErrorInvalidConfiguration;
    const unsigned wgs = (unsigned)((a.din + 1 + 63) / 64);
    hipLaunchKernelGGL(k_grad_softmax_bwd, dim3(wgs), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace bk
