// bk_eval.hip -- the convergence check, gfx950: one model
// scored on up to BK_EVAL_MAX_SETS resident sets, the counts returned.
//
// checkConvergence (DistSys/honest.go:141-162) calls testModel
// (honest.go:656-675: train_error / getTestErr) and, for the torch datasets,
// testAttackRate (honest.go:260-275: get17AttackRate) on the block's new model:
//     logistic  sum(sign(X . w) != y) / float(y.size)   (logistic_model_test.py:13-24)
//     softmax   1 - accuracy_score(argmax(model(x)), y) (ML/Pytorch/client.py:146-172)
// The arithmetic is the base-model evaluation of bk_roni / bk_roni_softmax
// (bk_roni.hip), bit for bit:
//
//   k_eval_sign    thread t of a workgroup takes sample t of its 256-sample
//                  tile: the dot as one fp64 FMA chain over k ascending from
//                  +0.0 (the chain K7's MFMAs round like), np.sign,
//                  the label compare.  d <= 32: the row straight into registers;
//                  beyond: through LDS in chunks of 32 features
//   k_eval_logits  a wave takes 16 samples x 16 class columns on
//                  v_mfma_f64_16x16x4_f64, a workgroup 64 samples.  The model's
//                  preparation is folded in: the weights are rounded to fp32 as
//                  they are staged, and wave 0 runs W W^T beside its logits,
//                  whose diagonal is k_roni_wnorm's sequential sum of squares
//
// Both take a descriptor table: a launch's workgroups index the concatenated
// sample tiles of every requested set.  Thread 0 of a workgroup adds its counts
// to the launch's counters and leaves through round_exit (bk_roni_dev.h); the
// last workgroup out writes every set's error, count and near ties into mapped
// host memory and zeroes the counters for the next launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <new>

#include "bk_ctx.h"
#include "bk_roni_dev.h"

namespace bk {

typedef double d4 __attribute__((ext_vector_type(4)));

// the set of workgroup blk and the first sample of its tile
__device__ inline int eval_find(const EvalDesc &desc, int blk, int tile_samples, int64_t *s0) {
    int si = 0, t0 = desc.s[0].tile0;  // tile0 ascends with the set
#pragma unroll
    for (int i = 1; i < EVAL_MAX_SETS; ++i)
        if (i < desc.nsets && blk >= desc.s[i].tile0) {
            si = i;
            t0 = desc.s[i].tile0;
        }
    *s0 = (int64_t)(blk - t0) * tile_samples;
    return si;
}

// the set's fields without a dynamic index into the kernel's arguments
__device__ inline EvalSet eval_pick(const EvalDesc &desc, int si) {
    EvalSet s;
    s.X = desc.s[0].X, s.y = desc.s[0].y, s.xn = desc.s[0].xn;
    s.nv = desc.s[0].nv, s.ldv = desc.s[0].ldv, s.tile0 = desc.s[0].tile0;
#pragma unroll
    for (int i = 1; i < EVAL_MAX_SETS; ++i) {
        const bool on = i == si;
        s.X = on ? desc.s[i].X : s.X;
        s.y = on ? desc.s[i].y : s.y;
        s.xn = on ? desc.s[i].xn : s.xn;
        s.nv = on ? desc.s[i].nv : s.nv;
        s.ldv = on ? desc.s[i].ldv : s.ldv;
        s.tile0 = on ? desc.s[i].tile0 : s.tile0;
    }
    return s;
}

// the last workgroup out: every set's totals into the mapped block, then the
// counters back to zero (nobody else is left to touch them)
__device__ inline void eval_write(const EvalDesc &desc, bool softmax, unsigned int *cnt,
                                  EvalOut *out) {
#pragma unroll
    for (int i = 0; i < EVAL_MAX_SETS; ++i) {
        if (i >= desc.nsets) break;
        const int64_t nv = desc.s[i].nv;
        const unsigned int a = round_load(cnt + i), nt = round_load(cnt + EVAL_MAX_SETS + i);
        const double dn = (double)nv;
        if (softmax) {  // k_roni_mc_score's expression
            out->err[i] = 1.0 - (double)a / dn;
            out->wrong[i] = nv - (int64_t)a;
        } else {  // k_roni_score's
            out->err[i] = (double)a / dn;
            out->wrong[i] = (int64_t)a;
        }
        out->near[i] = (int32_t)nt;
    }
    for (int i = 0; i <= EVAL_EXIT; ++i)
        __hip_atomic_store(cnt + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr int ES_KC = 32;

template <bool REG>
__global__ __launch_bounds__(256) void k_eval_sign(const EvalDesc desc, const double *__restrict__ ww,
                                                   int64_t din, unsigned int *__restrict__ cnt,
                                                   EvalOut *__restrict__ out) {
    __shared__ double xs[REG ? 1 : EVAL_SIGN_TS][ES_KC + 1];
    __shared__ double wsm[ES_KC];
    __shared__ unsigned int s_cnt;
    const int tid = threadIdx.x, l = tid & 63;
    int64_t s0;
    const int si = eval_find(desc, (int)blockIdx.x, EVAL_SIGN_TS, &s0);
    const EvalSet set = eval_pick(desc, si);
    const double *__restrict__ Xv = (const double *)set.X;
    const double *__restrict__ yv = (const double *)set.y;
    const int64_t nv = set.nv, ldv = set.ldv;
    if (tid == 0) s_cnt = 0;
    const int64_t s = s0 + tid, sc = s < nv ? s : nv - 1;
    double acc = 0.0;
    if (REG) {  // din <= 32: clamped loads, all in flight, then the chain
        const double *xr = Xv + sc * ldv;
        double x[ES_KC];
#pragma unroll
        for (int k = 0; k < ES_KC; ++k) x[k] = xr[k < din ? k : din - 1];
#pragma unroll
        for (int k = 0; k < ES_KC; ++k) {
            const double w = ww[k < din ? k : din - 1];
            acc = k < din ? __builtin_fma(x[k], w, acc) : acc;
        }
    } else {
        // staging: thread t moves feature t & 31 of samples (t >> 5) + 8 u
        // ([sample][k] row stride 33 doubles: conflict-free both ways), the
        // next chunk's loads in flight under this chunk's chain
        const int xk = tid & 31, xr = tid >> 5;
        double xv[ES_KC], wv = 0.0;
        auto load = [&](int64_t k0) {
            int64_t k = k0 + xk;
            k = k < din ? k : din - 1;
#pragma unroll
            for (int u = 0; u < ES_KC; ++u) {
                int64_t r = s0 + xr + 8 * u;
                r = r < nv ? r : nv - 1;
                xv[u] = Xv[r * ldv + k];
            }
            if (xr == 0) wv = ww[k];
        };
        load(0);
        for (int64_t k0 = 0; k0 < din; k0 += ES_KC) {
            __syncthreads();  // the previous chunk has been consumed
#pragma unroll
            for (int u = 0; u < ES_KC; ++u) xs[REG ? 0 : xr + 8 * u][xk] = xv[u];
            if (xr == 0) wsm[xk] = wv;
            __syncthreads();
            if (k0 + ES_KC < din) load(k0 + ES_KC);
            const int kn = (int)(din - k0 < ES_KC ? din - k0 : ES_KC);
            for (int kk = 0; kk < kn; ++kk) acc = __builtin_fma(xs[REG ? 0 : tid][kk], wsm[kk], acc);
        }
    }
    const double y = yv[sc];
    const double v = acc;  // np.sign: 0 -> 0, NaN -> NaN
    const double yh = v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : (v == 0.0 ? 0.0 : v));
    const unsigned int mis = (unsigned int)__popcll(__ballot(s < nv && !(yh == y)));
    __syncthreads();  // s_cnt is zero
    if (l == 0 && mis) atomicAdd(&s_cnt, mis);
    __syncthreads();
    if (tid != 0) return;
    const unsigned int mine[1] = {s_cnt};
    const int slot[1] = {si};
    if (!round_exit(mine, slot, cnt, EVAL_EXIT)) return;
    eval_write(desc, false, cnt, out);
}

// k_eval_logits: the samples and the model's 16 class rows (fp32, rows past C
// and features past d_in zero) go through LDS in chunks of 64 features (row
// stride 68 floats: an A / B fragment's 16 rows x 4 k hit distinct banks), the
// next chunk's loads in flight under this chunk's MFMAs.  Per k-step of 4 a
// wave issues one MFMA (A: its 16 samples, B: the 16 classes), wave 0 a second
// one (A = B = the classes).  D reg r of lane l is row (l >> 4) + 4 r, column
// l & 15.  Then logit = fp32(acc + b) into LDS, and lane s of wave 0 takes
// np.argmax, the label compare and softmax_near_tie for sample s: K8's epilogue.
constexpr int EL_KC = 64, EL_XS = 68;

__global__ __launch_bounds__(256) void k_eval_logits(const EvalDesc desc,
                                                     const double *__restrict__ ww, int64_t din,
                                                     int C, double g, unsigned int *__restrict__ cnt,
                                                     EvalOut *__restrict__ out) {
    __shared__ float xs[EVAL_LOGITS_TS][EL_XS];
    __shared__ float wsf[16][EL_XS];
    __shared__ float lt[EVAL_LOGITS_TS][17];
    __shared__ double bl[16], wnl[16];
    const int tid = threadIdx.x, l = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int64_t s0;
    const int si = eval_find(desc, (int)blockIdx.x, EVAL_LOGITS_TS, &s0);
    const EvalSet set = eval_pick(desc, si);
    const float *__restrict__ Xv = (const float *)set.X;
    const int32_t *__restrict__ yv = (const int32_t *)set.y;
    const int64_t nv = set.nv, ldv = set.ldv;
    if (tid < 16)  // the model's fp32 biases
        bl[tid] = tid < C ? (double)(float)ww[(int64_t)C * din + tid] : 0.0;
    // staging: thread t moves feature t & 63 of samples / classes (t >> 6) + 4 u
    const int xk = tid & 63, xr = tid >> 6;
    float xv[16], wv[4];
    auto load = [&](int64_t k0) {  // clamped addresses, every load in flight
        const int64_t k = k0 + xk;
        const bool kin = k < din;
        const int64_t kc = kin ? k : din - 1;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            int64_t s = s0 + xr + 4 * u;
            s = s < nv ? s : nv - 1;
            const float x = Xv[s * ldv + kc];
            xv[u] = kin ? x : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = xr + 4 * u;
            const double w = ww[(int64_t)(c < C ? c : C - 1) * din + kc];
            wv[u] = kin && c < C ? (float)w : 0.0f;
        }
    };
    d4 acc = d4{0.0, 0.0, 0.0, 0.0}, accw = d4{0.0, 0.0, 0.0, 0.0};
    const int arow = 16 * wave + (l & 15), ak = l >> 4;
    load(0);
    for (int64_t k0 = 0; k0 < din; k0 += EL_KC) {
        __syncthreads();  // the previous chunk has been consumed
#pragma unroll
        for (int u = 0; u < 16; ++u) xs[xr + 4 * u][xk] = xv[u];
#pragma unroll
        for (int u = 0; u < 4; ++u) wsf[xr + 4 * u][xk] = wv[u];
        __syncthreads();
        if (k0 + EL_KC < din) load(k0 + EL_KC);
        const int kn = (int)(din - k0 < EL_KC ? din - k0 : EL_KC);
        const int steps = (kn + 3) >> 2;  // features past d_in are zero in LDS
        for (int st = 0; st < steps; ++st) {
            const double a = (double)xs[arow][4 * st + ak];
            const double b = (double)wsf[l & 15][4 * st + ak];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
            if (wave == 0) accw = __builtin_amdgcn_mfma_f64_16x16x4f64(b, b, accw, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
        lt[16 * wave + (l >> 4) + 4 * r][l & 15] = (float)(acc[r] + bl[l & 15]);
    if (wave == 0) {  // the diagonal of W W^T: class c in lane (c & 3) 16 + c, reg c >> 2
        const int c = l & 15;
        if ((l >> 4) == (c & 3)) {
            const int r = c >> 2;
            const double q = r == 0 ? accw[0] : r == 1 ? accw[1] : r == 2 ? accw[2] : accw[3];
            wnl[c] = __builtin_sqrt(q);
        }
    }
    __syncthreads();
    if (tid >= 64) return;  // wave 0: lane s takes sample s (no barrier below)
    const int64_t s = s0 + l, sc = s < nv ? s : nv - 1;
    // np.argmax: the first maximum, a NaN wins at its first place
    const float *lg = lt[l];
    int best = 0;
    float b0 = lg[0];
    for (int c = 1; c < C; ++c) {
        const float v = lg[c];
        if (!(b0 != b0) && (v != v || v > b0)) {
            best = c;
            b0 = v;
        }
    }
    const bool ok = s < nv && best == yv[sc];
    const bool nt = s < nv && softmax_near_tie(lg, C, best, set.xn[sc], wnl, bl, g);
    const unsigned int mine[2] = {(unsigned int)__popcll(__ballot(ok)),
                                  (unsigned int)__popcll(__ballot(nt))};
    if (tid != 0) return;
    const int slot[2] = {si, EVAL_MAX_SETS + si};
    if (!round_exit(mine, slot, cnt, EVAL_EXIT)) return;
    eval_write(desc, true, cnt, out);
}

hipError_t launch_eval_sign(const EvalDesc &desc, int tiles, const double *ww, int64_t d,
                            unsigned int *cnt, EvalOut *out, hipStream_t st) {
    if (tiles < 1 || desc.nsets < 1 || desc.nsets > EVAL_MAX_SETS) return hipErrorInvalidConfiguration;
    if (d <= ES_KC)
        hipLaunchKernelGGL(k_eval_sign<true>, dim3((unsigned)tiles), dim3(256), 0, st, desc, ww, d, cnt,
                           out);
    else
        hipLaunchKernelGGL(k_eval_sign<false>, dim3((unsigned)tiles), dim3(256), 0, st, desc, ww, d,
                           cnt, out);
    return hipGetLastError();
}

hipError_t launch_eval_logits(const EvalDesc &desc, int tiles, const double *ww, int64_t din, int C,
                              unsigned int *cnt, EvalOut *out, hipStream_t st) {
    if (tiles < 1 || desc.nsets < 1 || desc.nsets > EVAL_MAX_SETS || C < 2 || C > 16)
        return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_eval_logits, dim3((unsigned)tiles), dim3(256), 0, st, desc, ww, din, C,
                       roni_softmax_g(din), cnt, out);
    return hipGetLastError();
}

// ---- the host side ----------------------------------------------------------
void eval_destroy(Eval *e) {
    if (!e) return;
    for (EvalSlot &s : e->set)
        for (DevBuf *b : {&s.X, &s.y, &s.xn})
            if (b->p) (void)hipFree(b->p);
    for (DevBuf *b : {&e->w, &e->cnt})
        if (b->p) (void)hipFree(b->p);
    if (e->out) (void)hipHostFree(e->out);
    delete e;
}

static int eval_state(bk_ctx *c) {
    if (c->eval) return BK_OK;
    c->eval = new (std::nothrow) Eval();
    if (!c->eval) return fail(BK_ENOMEM, "host allocation of the evaluation sets failed");
    return BK_OK;
}

static int check_set_index(int set) {
    if (set < 0 || set >= EVAL_MAX_SETS)
        return fail(BK_EINVAL, "set=%d outside [0, %d)", set, EVAL_MAX_SETS);
    return BK_OK;
}

static int check_set_shape(int64_t nv, int64_t d, int64_t ldv) {
    if (nv < 1 || d < 1) return fail(BK_EINVAL, "need nv >= 1 and d >= 1 (nv=%lld, d=%lld)",
                                     (long long)nv, (long long)d);
    if (ldv < d) return fail(BK_EINVAL, "ldv=%lld < d=%lld", (long long)ldv, (long long)d);
    if (nv > ((int64_t)1 << 31)) return fail(BK_ENOTSUP, "nv=%lld too large", (long long)nv);
    if (d > ((int64_t)1 << 21)) return fail(BK_ENOTSUP, "d=%lld exceeds 2^21", (long long)d);
    return BK_OK;
}

int eval_check_args(const int *sets, int nsets, const double *err, const int64_t *wrong) {
    if (!sets || !err || !wrong) return fail(BK_EINVAL, "null sets / err / wrong");
    if (nsets < 1 || nsets > EVAL_MAX_SETS)
        return fail(BK_EINVAL, "nsets=%d outside [1, %d]", nsets, EVAL_MAX_SETS);
    for (int i = 0; i < nsets; ++i) CHK(check_set_index(sets[i]));
    return BK_OK;
}

int eval_check_sets(bk_ctx *c, int64_t d, const int *sets, int nsets) {
    int kind = EVAL_EMPTY;
    for (int i = 0; i < nsets; ++i) {
        const EvalSlot *s = c->eval ? &c->eval->set[sets[i]] : nullptr;
        if (!s || s->kind == EVAL_EMPTY)
            return fail(BK_EINVAL, "evaluation set %d is empty: call bk_eval_set_*", sets[i]);
        if (kind != EVAL_EMPTY && s->kind != kind)
            return fail(BK_EINVAL, "evaluation set %d is of another kind than set %d", sets[i],
                        sets[0]);
        kind = s->kind;
        if (s->d != d)
            return fail(BK_EINVAL, "d=%lld != evaluation set %d's %lld", (long long)d, sets[i],
                        (long long)s->d);
        for (int j = 0; j < i; ++j)
            if (sets[j] == sets[i]) return fail(BK_EINVAL, "evaluation set %d is named twice", sets[i]);
    }
    return BK_OK;
}

// the launch's counters (zeroed once: every launch leaves them zero) and the
// mapped block its last workgroup writes
static int ensure_eval_out(bk_ctx *c, Eval *e) {
    if (!e->cnt.p) {
        CHK(ensure(e->cnt, EVAL_CNT_WORDS * sizeof(unsigned int)));
        HIPCHK(hipMemsetAsync(e->cnt.p, 0, EVAL_CNT_WORDS * sizeof(unsigned int), c->stream));
    }
    if (!e->out) {
        void *h = nullptr, *d = nullptr;
        HIPCHK(hipHostMalloc(&h, 4096,
                             hipHostMallocPortable | hipHostMallocMapped | hipHostMallocNonCoherent));
        if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
            (void)hipHostFree(h);
            return fail(BK_EHIP, "hipHostGetDevicePointer failed for the evaluation block");
        }
        e->out = (EvalOut *)h;
        e->out_dev = (EvalOut *)d;
    }
    return BK_OK;
}

int eval_queue(bk_ctx *c, const double *dw, const int *sets, int nsets) {
    Eval *e = c->eval;
    CHK(ensure_eval_out(c, e));
    const EvalSlot &first = e->set[sets[0]];
    const bool softmax = first.kind == EVAL_SOFTMAX;
    const int ts = softmax ? EVAL_LOGITS_TS : EVAL_SIGN_TS;
    EvalDesc desc = {};
    desc.nsets = nsets;
    int64_t tiles = 0;
    for (int i = 0; i < nsets; ++i) {
        const EvalSlot &s = e->set[sets[i]];
        desc.s[i] = {s.X.p, s.y.p, (const double *)s.xn.p, s.nv, softmax ? s.din : s.d, (int)tiles};
        tiles += (s.nv + ts - 1) / ts;
        if (tiles > 0x7fffffff) return fail(BK_ENOTSUP, "the sets' %lld tiles exceed the grid",
                                            (long long)tiles);
    }
    const hipError_t he =
        softmax ? launch_eval_logits(desc, (int)tiles, dw, first.din, (int)first.C,
                                     (unsigned int *)e->cnt.p, e->out_dev, c->stream)
                : launch_eval_sign(desc, (int)tiles, dw, first.d, (unsigned int *)e->cnt.p, e->out_dev,
                                   c->stream);
    if (he != hipSuccess) return fail(BK_EHIP, "k_eval launch: %s", hipGetErrorString(he));
    ++e->launches;
    return BK_OK;
}

void eval_collect(bk_ctx *c, int nsets, double *err, int64_t *wrong, int32_t *near_ties) {
    const EvalOut *o = c->eval->out;
    memcpy(err, o->err, (size_t)nsets * sizeof(double));
    memcpy(wrong, o->wrong, (size_t)nsets * sizeof(int64_t));
    if (near_ties) memcpy(near_ties, o->near, (size_t)nsets * sizeof(int32_t));
    ++c->eval->calls;
}

}  // namespace bk

int bk_eval_set_logistic(bk_ctx *c, int set, const double *X, int64_t nv, int64_t d, int64_t ldv,
                         const double *y) {
    if (!c) return fail(BK_EINVAL, "null context");
    CHK(check_set_index(set));
    CHK(check_set_shape(nv, d, ldv));
    if (!X || !y) return fail(BK_EINVAL, "null X / y");
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    CHK(eval_state(c));
    EvalSlot &s = c->eval->set[set];
    s.kind = EVAL_EMPTY;  // empty until the new set has landed
    HostDrain drain{c};
    CHK(ensure(s.X, (size_t)nv * d * sizeof(double)));
    CHK(ensure(s.y, (size_t)nv * sizeof(double)));
    HIPCHK(hipMemcpy2DAsync(s.X.p, (size_t)d * sizeof(double), X, (size_t)ldv * sizeof(double),
                            (size_t)d * sizeof(double), (size_t)nv, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s.y.p, y, (size_t)nv * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    drain.armed = false;
    s.nv = nv;
    s.d = d;
    s.din = s.C = 0;
    s.kind = EVAL_LOGISTIC;
    return BK_OK;
}

int bk_eval_set_softmax(bk_ctx *c, int set, const float *X, int64_t nv, int64_t d_in, int64_t ldv,
                        const int32_t *y, int64_t n_classes) {
    if (!c) return fail(BK_EINVAL, "null context");
    CHK(check_set_index(set));
    CHK(check_set_shape(nv, d_in, ldv));
    if (n_classes < 2) return fail(BK_EINVAL, "n_classes=%lld < 2", (long long)n_classes);
    if (n_classes > 16) return fail(BK_ENOTSUP, "n_classes=%lld exceeds 16", (long long)n_classes);
    if (!X || !y) return fail(BK_EINVAL, "null X / y");
    for (int64_t i = 0; i < nv; ++i)
        if (y[i] < 0 || y[i] >= n_classes)
            return fail(BK_EINVAL, "label y[%lld]=%d outside [0, %lld)", (long long)i, (int)y[i],
                        (long long)n_classes);
    std::lock_guard<std::mutex> lk(c->mu);
    DeviceGuard dg(c->device);
    CHK(eval_state(c));
    EvalSlot &s = c->eval->set[set];
    s.kind = EVAL_EMPTY;
    HostDrain drain{c};
    CHK(ensure(s.X, (size_t)nv * d_in * sizeof(float)));
    CHK(ensure(s.y, (size_t)nv * sizeof(int32_t)));
    CHK(ensure(s.xn, (size_t)nv * sizeof(double)));
    HIPCHK(hipMemcpy2DAsync(s.X.p, (size_t)d_in * sizeof(float), X, (size_t)ldv * sizeof(float),
                            (size_t)d_in * sizeof(float), (size_t)nv, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s.y.p, y, (size_t)nv * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    // the samples' norms (the near-tie bound), once per set: K8's own kernel
    HIPCHK(launch_roni_xnorm((const float *)s.X.p, nv, d_in, d_in, (double *)s.xn.p, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    drain.armed = false;
    s.nv = nv;
    s.din = d_in;
    s.C = n_classes;
    s.d = n_classes * (d_in + 1);
    s.kind = EVAL_SOFTMAX;
    return BK_OK;
}

int bk_eval_clear(bk_ctx *c, int set) {
    if (!c) return fail(BK_EINVAL, "null context");
    CHK(check_set_index(set));
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->eval) c->eval->set[set].kind = EVAL_EMPTY;  // the buffers stay for the next set
    return BK_OK;
}

int bk_eval(bk_ctx *c, const double *ww, int64_t d, int where, const int *sets, int nsets,
            double *err, int64_t *wrong, int32_t *near_ties) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!ww) return fail(BK_EINVAL, "null ww");
    CHK(eval_check_args(sets, nsets, err, wrong));
    if (where != BK_HOST && where != BK_HOST_PINNED && where != BK_DEVICE)
        return fail(BK_EINVAL, "bad where=%d", where);
    std::lock_guard<std::mutex> lk(c->mu);
    CHK(eval_check_sets(c, d, sets, nsets));
    DeviceGuard dg(c->device);
    HostDrain drain{c};  // error returns: the queued copy may still read ww
    const double *dw = ww;
    if (where != BK_DEVICE) {
        CHK(ensure(c->eval->w, (size_t)d * sizeof(double)));
        CHK(timed(c, BK_K_H2D, [&] {
            return hipMemcpyAsync(c->eval->w.p, ww, (size_t)d * sizeof(double), hipMemcpyHostToDevice,
                                  c->stream);
        }));
        dw = (const double *)c->eval->w.p;
    }
    CHK(eval_queue(c, dw, sets, nsets));
    HIPCHK(wait_stream(c));
    drain.armed = false;
    eval_collect(c, nsets, err, wrong, near_ties);
    return BK_OK;
}

int bk_eval_stats(bk_ctx *c, int64_t out[2]) {
    if (!c) return fail(BK_EINVAL, "null context");
    if (!out) return fail(BK_EINVAL, "null out");
    std::lock_guard<std::mutex> lk(c->mu);
    out[0] = c->eval ? c->eval->launches : 0;
    out[1] = c->eval ? c->eval->calls : 0;
    return BK_OK;
}
