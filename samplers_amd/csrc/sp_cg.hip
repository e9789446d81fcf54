// The proximal data step by conjugate gradients, for every linear kind (sp_op_prox_cg_ws,
// sp_diffpir_step_cg_ws): regularised CGLS on (A^T A + rho I) z = A^T y + rho x0 in d = z - x0,
// with a stop of its own per sample (semantics: DESIGN.md §3, tests/prox_cg_ref.py):
//
//   s = y - A x0;  d = 0;  g = A^T s;  p = g;  gamma = |g|^2;  gamma0 = gamma;  iters = 0
//   K times:  q = A p;  delta = |q|^2 + rho |p|^2
//             live = gamma > tol^2 gamma0  and  delta > 0  and  gamma, delta finite
//             live:  alpha = gamma / delta;  d += alpha p;  s -= alpha q;  g = A^T s - rho d
//                    gamma' = |g|^2;  p = g + (gamma' / gamma) p;  gamma = gamma';  iters += 1
//             else:  nothing of the sample changes (a select, never a product by 0)
//   z = x0 + d
//
// A and A^T are the kind's own maps, called through its table row (sp_ops.h); this file is the
// vector side.  Launch sequence of a call, of fixed length whatever the samples do:
//   [head]  A  residual  A^T  init   K x ( A  qq  yupd  A^T  xupd  pupd )   tail
// (the last iteration's pupd is left out: p is not read again).  Memory model as sp_dps.hip: a
// block covers kIter * kBlock * V consecutive elements of ONE sample, grid = (tiles, batch), every
// squared norm is one partial per block, summed by block_sum_partials in its fixed order by every
// block that needs the total: no atomics, no grid barrier, no host round trip.  yupd's block 0
// leaves the sample's scalars (gamma, alpha, live, iters) in a 16-byte record that the two
// x-space launches after it read; nothing reads a record in the launch that writes it.  A sample
// is computed alone, so its bits do not depend on the batch, y_div or the other samples' stops.
//
// Bytes per iteration and sample outside the maps: qq 4m, yupd 12m (s, q read, s written), xupd
// 20n (d, p, A^T s read, d, g written), pupd 12n: 16m + 32n, plus the partials.

#include <cmath>

#define SP_TU 23  // debug-build site numbering (sp_common.h SP_DCHECK)
#include "sp_ops.h"

namespace sp {

// the scalars of one sample between launches (work, behind the partials)
struct cg_state {
    float gamma, alpha;
    int32_t live, iters;
};
static_assert(sizeof(cg_state) == 16, "four words per sample (sp_prox_cg_workspace)");

// where the pieces of `work` lie for one call; every piece starts on a multiple of four floats
struct cg_layout {
    int64_t vec_n, vec_m;  // floats of one x-space / y-space vector, rounded up
    int Pn, Pm;
    float *d, *p, *g, *x0, *s, *q;  // x0: the step form's own; the prox form reads the caller's
    float *part_g, *part_g0, *part_p, *part_q;
    cg_state* st;
    float* op_work;
    int64_t floats;
};

static int64_t round4(int64_t v) { return (v + 3) & ~int64_t(3); }

static cg_layout cg_plan(const sp_op* op, int64_t batch, bool step_form, float* work) {
    cg_layout L;
    L.vec_n = round4(batch * op->n), L.vec_m = round4(batch * op->m);
    L.Pn = static_cast<int>(tiles_elementwise(op->n)), L.Pm = static_cast<int>(tiles_elementwise(op->m));
    int64_t o = 0;
    auto take = [&](int64_t count) { float* r = work ? work + o : nullptr; o += count; return r; };
    L.d = take(L.vec_n), L.p = take(L.vec_n), L.g = take(L.vec_n);
    L.x0 = step_form ? take(L.vec_n) : nullptr;
    L.s = take(L.vec_m), L.q = take(L.vec_m);
    float* parts = take(round4(batch * (3 * (int64_t)L.Pn + L.Pm)));
    L.part_g = parts;
    L.part_g0 = parts ? parts + batch * L.Pn : nullptr;
    L.part_p = parts ? parts + 2 * batch * L.Pn : nullptr;
    L.part_q = parts ? parts + 3 * batch * L.Pn : nullptr;
    L.st = reinterpret_cast<cg_state*>(take(4 * batch));
    L.op_work = take(0);
    const op_kind* k = kind_of(op);
    L.floats = o + (k->op_workspace ? k->op_workspace(op, batch) : 0);
    return L;
}

// PHASE, the one nonlinear kind, has the _ws pair too
static bool cg_serves(const sp_op* op) {
    const op_kind* k = kind_of(op);
    return (k->apply && k->adjoint) || (k->apply_ws && k->vjp_ws && op->kind != SP_OP_PHASE);
}

static int cg_apply(const sp_op* op, const float* x, float* y, int64_t batch, float* op_work, hipStream_t s) {
    const op_kind* k = kind_of(op);
    return k->apply_ws ? k->apply_ws(op, x, y, batch, op_work, s) : k->apply(op, x, y, batch, s);
}

static int cg_adjoint(const sp_op* op, const float* y, float* x, int64_t batch, float* op_work, hipStream_t s) {
    const op_kind* k = kind_of(op);  // the linear kinds' vjp_ws does not read its x argument
    return k->vjp_ws ? k->vjp_ws(op, y, y, x, batch, op_work, s) : k->adjoint(op, y, x, batch, s);
}

// element index of thread's group `it` in its block's tile
template <int V>
__device__ __forceinline__ int64_t tile_index(int it) {
    return ((int64_t)blockIdx.x * kIter + it) * (kBlock * V) + threadIdx.x * V;
}

// ---------------------------------------------------------------------------
// head (step form): x0 = (x - k eps) / a, the reciprocal taken once as k_prox takes it
// ---------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(kBlock) void k_cg_head(const float* __restrict__ x,
                                                    const float* __restrict__ eps, int64_t n, float a,
                                                    float k, float* __restrict__ x0) {
#pragma clang fp contract(off)
    const int64_t b = blockIdx.y;
    const float inv_a = 1.f / a;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int64_t j = tile_index<V>(it);
        if (j < n) {
            SP_DCHECK(j + V <= n);
            float xv[V], ev[V], o[V];
            load_v<V>(x + b * n + j, xv);
            load_v<V>(eps + b * n + j, ev);
#pragma unroll
            for (int e = 0; e < V; ++e) o[e] = (xv[e] - k * ev[e]) * inv_a;
            store_v<V>(x0 + b * n + j, o);
        }
    }
}

// s = y[b / y_div] - q
template <int V>
__global__ __launch_bounds__(kBlock) void k_cg_residual(const float* __restrict__ y,
                                                        const float* __restrict__ q, int64_t m,
                                                        int64_t y_div, float* __restrict__ s) {
    const int64_t b = blockIdx.y;
    const float* yb = y + (b / y_div) * m;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int64_t j = tile_index<V>(it);
        if (j < m) {
            SP_DCHECK(j + V <= m);
            float yv[V], qv[V], o[V];
            load_v<V>(yb + j, yv);
            load_v<V>(q + b * m + j, qv);
#pragma unroll
            for (int e = 0; e < V; ++e) o[e] = yv[e] - qv[e];
            store_v<V>(s + b * m + j, o);
        }
    }
}

// d = 0, p = g, the |g|^2 partials into gamma, gamma0 and |p|^2; the sample's record cleared
template <int V>
__global__ __launch_bounds__(kBlock) void k_cg_init(const float* __restrict__ g, int64_t n, int P,
                                                    float* __restrict__ d, float* __restrict__ p,
                                                    float* __restrict__ part_g,
                                                    float* __restrict__ part_g0,
                                                    float* __restrict__ part_p,
                                                    cg_state* __restrict__ st) {
#pragma clang fp contract(off)
    __shared__ float red[4];
    const int64_t b = blockIdx.y;
    float acc = 0.f;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int64_t j = tile_index<V>(it);
        if (j < n) {
            SP_DCHECK(j + V <= n);
            float gv[V], zero[V] = {};
            load_v<V>(g + b * n + j, gv);
#pragma unroll
            for (int e = 0; e < V; ++e) acc += gv[e] * gv[e];
            store_v<V>(d + b * n + j, zero);
            store_v<V>(p + b * n + j, gv);
        }
    }
    const float t = block_sum(acc, red);
    SP_DCHECK(static_cast<int>(blockIdx.x) < P);
    if (threadIdx.x == 0) {
        const int64_t i = b * P + blockIdx.x;
        part_g[i] = t, part_g0[i] = t, part_p[i] = t;
        if (blockIdx.x == 0) st[b] = cg_state{0.f, 0.f, 0, 0};
    }
}

// the |q|^2 partials
template <int V>
__global__ __launch_bounds__(kBlock) void k_cg_qq(const float* __restrict__ q, int64_t m, int P,
                                                  float* __restrict__ part_q) {
#pragma clang fp contract(off)
    __shared__ float red[4];
    const int64_t b = blockIdx.y;
    float acc = 0.f;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int64_t j = tile_index<V>(it);
        if (j < m) {
            SP_DCHECK(j + V <= m);
            float qv[V];
            load_v<V>(q + b * m + j, qv);
#pragma unroll
            for (int e = 0; e < V; ++e) acc += qv[e] * qv[e];
        }
    }
    const float t = block_sum(acc, red);
    SP_DCHECK(static_cast<int>(blockIdx.x) < P);
    if (threadIdx.x == 0) part_q[b * P + blockIdx.x] = t;
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e+38f; }  // NaN fails

// the y-space update: every block sums the sample's four partial arrays in block_sum_partials'
// order, so all of them take the same decision; live: s -= alpha q.  Block 0 records the scalars.
template <int V>
__global__ __launch_bounds__(kBlock) void k_cg_yupd(const float* __restrict__ q, int64_t m, int Pm,
                                                    int Pn, const float* __restrict__ part_g,
                                                    const float* __restrict__ part_g0,
                                                    const float* __restrict__ part_p,
                                                    const float* __restrict__ part_q, float rho,
                                                    float tol, float* __restrict__ s,
                                                    cg_state* __restrict__ st) {
#pragma clang fp contract(off)
    __shared__ float red[4][4];
    const int64_t b = blockIdx.y;
    SP_DCHECK(static_cast<int>(blockIdx.x) < Pm && Pn > 0);
    const float gamma = block_sum_partials(part_g + b * Pn, Pn, red[0]);
    const float gamma0 = block_sum_partials(part_g0 + b * Pn, Pn, red[1]);
    const float pp = block_sum_partials(part_p + b * Pn, Pn, red[2]);
    const float qq = block_sum_partials(part_q + b * Pm, Pm, red[3]);
    const float delta = qq + rho * pp;
    const bool live = gamma > (tol * tol) * gamma0 && delta > 0.f && finite_f(gamma) && finite_f(delta);
    const float alpha = gamma / delta;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        cg_state r = st[b];  // iters alone is carried over; no other block reads the record here
        r.gamma = gamma, r.alpha = alpha, r.live = live ? 1 : 0, r.iters += live ? 1 : 0;
        st[b] = r;
    }
    if (!live) return;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int64_t j = tile_index<V>(it);
        if (j < m) {
            SP_DCHECK(j + V <= m);
            float sv[V], qv[V];
            load_v<V>(s + b * m + j, sv);
            load_v<V>(q + b * m + j, qv);
#pragma unroll
            for (int e = 0; e < V; ++e) sv[e] = sv[e] - alpha * qv[e];
            store_v<V>(s + b * m + j, sv);
        }
    }
}

// the x-space update of a live sample: d += alpha p, g = A^T s - rho d in place, gamma' partials
template <int V>
__global__ __launch_bounds__(kBlock) void k_cg_xupd(const float* __restrict__ p, int64_t n, int P,
                                                    float rho, const cg_state* __restrict__ st,
                                                    float* __restrict__ d, float* __restrict__ g,
                                                    float* __restrict__ part_g) {
#pragma clang fp contract(off)
    __shared__ float red[4];
    const int64_t b = blockIdx.y;
    const cg_state r = st[b];
    if (!r.live) return;  // the whole block: the record is the sample's
    float acc = 0.f;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int64_t j = tile_index<V>(it);
        if (j < n) {
            SP_DCHECK(j + V <= n);
            float dv[V], pv[V], gv[V];
            load_v<V>(d + b * n + j, dv);
            load_v<V>(p + b * n + j, pv);
            load_v<V>(g + b * n + j, gv);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                dv[e] = dv[e] + r.alpha * pv[e];
                gv[e] = gv[e] - rho * dv[e];
                acc += gv[e] * gv[e];
            }
            store_v<V>(d + b * n + j, dv);
            store_v<V>(g + b * n + j, gv);
        }
    }
    const float t = block_sum(acc, red);
    SP_DCHECK(static_cast<int>(blockIdx.x) < P);
    if (threadIdx.x == 0) part_g[b * P + blockIdx.x] = t;
}

// the direction update of a live sample: beta = gamma' / gamma, p = g + beta p, |p|^2 partials
template <int V>
__global__ __launch_bounds__(kBlock) void k_cg_pupd(const float* __restrict__ g, int64_t n, int P,
                                                    const cg_state* __restrict__ st,
                                                    const float* __restrict__ part_g,
                                                    float* __restrict__ p,
                                                    float* __restrict__ part_p) {
#pragma clang fp contract(off)
    __shared__ float red[4], redp[4];
    const int64_t b = blockIdx.y;
    const cg_state r = st[b];
    if (!r.live) return;
    SP_DCHECK(static_cast<int>(blockIdx.x) < P);
    const float beta = block_sum_partials(part_g + b * P, P, redp) / r.gamma;
    float acc = 0.f;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int64_t j = tile_index<V>(it);
        if (j < n) {
            SP_DCHECK(j + V <= n);
            float gv[V], pv[V];
            load_v<V>(g + b * n + j, gv);
            load_v<V>(p + b * n + j, pv);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                pv[e] = gv[e] + beta * pv[e];
                acc += pv[e] * pv[e];
            }
            store_v<V>(p + b * n + j, pv);
        }
    }
    const float t = block_sum(acc, red);
    if (threadIdx.x == 0) part_p[b * P + blockIdx.x] = t;
}

// ---------------------------------------------------------------------------
// tail: z = x0 + d (x0 itself where no iteration ran); STEP: eps_hat = (x - a z) / k and
// x' = a_prev z + (c_eps eps_hat + c_xi xi), xi read or drawn as k_prox draws it
// ---------------------------------------------------------------------------
template <int V, bool STEP, bool XI_IN>
__global__ __launch_bounds__(kBlock) void k_cg_tail(const float* __restrict__ x0,
                                                    const float* __restrict__ d,
                                                    const float* __restrict__ x,
                                                    const float* __restrict__ xi, uint64_t seed,
                                                    int64_t step, int64_t sample_offset, int64_t n,
                                                    sp_prox_coefs c, const cg_state* __restrict__ st,
                                                    float* __restrict__ out,
                                                    int32_t* __restrict__ iters_out) {
#pragma clang fp contract(off)
    const int64_t b = blockIdx.y;
    const int32_t iters = st[b].iters;
    if (iters_out && blockIdx.x == 0 && threadIdx.x == 0) iters_out[b] = iters;
    const float inv_k = STEP ? 1.f / c.k : 1.f;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int64_t j = tile_index<V>(it);
        if (j < n) {
            SP_DCHECK(j + V <= n);
            float x0v[V], dv[V], xv[V], nz[V] = {}, o[V];
            load_v<V>(x0 + b * n + j, x0v);
            load_v<V>(d + b * n + j, dv);
            if constexpr (STEP) {
                load_v<V>(x + b * n + j, xv);
                noise_v<V, XI_IN>(xi, seed, step, sample_offset, b, n, j, nz);
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float z = iters > 0 ? x0v[e] + dv[e] : x0v[e];
                o[e] = STEP ? diffpir_update(c, inv_k, xv[e], z, nz[e]) : z;
            }
            store_v<V>(out + b * n + j, o);
        }
    }
}

// ---------------------------------------------------------------------------
// the launch sequence
// ---------------------------------------------------------------------------
struct cg_args {
    const float *x, *eps, *y, *xi;  // eps null: the prox form, x holds x0
    uint64_t seed;
    int64_t step, sample_offset, batch, y_div;
    sp_prox_coefs c;
    int32_t max_iter;
    float tol;
    float* out;
    int32_t* iters_out;
    float* work;
};

#define SP_CG_V(V4, KERNEL, ...)                                       \
    do {                                                               \
        if (V4) launch(0, KERNEL<4>, __VA_ARGS__);                     \
        else launch(0, KERNEL<1>, __VA_ARGS__);                        \
    } while (0)

static int cg_run(const sp_op* op, const cg_args& a, hipStream_t s) {
    const char* what = a.eps ? "sp_diffpir_step_cg_ws" : "sp_op_prox_cg_ws";
    const bool step_form = a.eps != nullptr;
    const cg_layout L = cg_plan(op, a.batch, step_form, a.work);
    const int64_t n = op->n, m = op->m, B = a.batch;
    const bool vn = n % 4 == 0, vm = m % 4 == 0;
    const dim3 gn = sample_grid(L.Pn, B), gm = sample_grid(L.Pm, B), blk(kBlock);
    const float rho = a.c.rho;
    int rc;
    const float* x0 = a.x;
    if (step_form) {
        SP_CG_V(vn, k_cg_head, gn, blk, s, a.x, a.eps, n, a.c.a, a.c.k, L.x0);
        x0 = L.x0;
    }
    if ((rc = cg_apply(op, x0, L.q, B, L.op_work, s)) != SP_OK) return rc;
    SP_CG_V(vm, k_cg_residual, gm, blk, s, a.y, (const float*)L.q, m, a.y_div, L.s);
    if ((rc = cg_adjoint(op, L.s, L.g, B, L.op_work, s)) != SP_OK) return rc;
    SP_CG_V(vn, k_cg_init, gn, blk, s, (const float*)L.g, n, L.Pn, L.d, L.p, L.part_g, L.part_g0,
            L.part_p, L.st);
    for (int32_t i = 0; i < a.max_iter; ++i) {
        if ((rc = cg_apply(op, L.p, L.q, B, L.op_work, s)) != SP_OK) return rc;
        SP_CG_V(vm, k_cg_qq, gm, blk, s, (const float*)L.q, m, L.Pm, L.part_q);
        SP_CG_V(vm, k_cg_yupd, gm, blk, s, (const float*)L.q, m, L.Pm, L.Pn, (const float*)L.part_g,
                (const float*)L.part_g0, (const float*)L.part_p, (const float*)L.part_q, rho, a.tol,
                L.s, L.st);
        if ((rc = cg_adjoint(op, L.s, L.g, B, L.op_work, s)) != SP_OK) return rc;
        SP_CG_V(vn, k_cg_xupd, gn, blk, s, (const float*)L.p, n, L.Pn, rho, (const cg_state*)L.st,
                L.d, L.g, L.part_g);
        if (i + 1 < a.max_iter)
            SP_CG_V(vn, k_cg_pupd, gn, blk, s, (const float*)L.g, n, L.Pn, (const cg_state*)L.st,
                    (const float*)L.part_g, L.p, L.part_p);
    }
    select_width(n, [&](auto v) {
        select_bool(step_form, [&](auto step) {
            select_bool(a.xi, [&](auto xin) {  // the prox form has no noise: one kernel
                launch(0, k_cg_tail<v(), step(), step() && xin()>, gn, blk, s, x0, (const float*)L.d,
                       a.x, a.xi, a.seed, a.step, a.sample_offset, n, a.c, (const cg_state*)L.st,
                       a.out, a.iters_out);
            });
        });
    });
    return check_launch(what);
}
#undef SP_CG_V

static bool cg_scalars_ok(float rho, int32_t max_iter, float tol) {
    return rho > 0.f && rho <= 3.402823466e+38f && max_iter >= 1 && tol >= 0.f &&
           tol <= 3.402823466e+38f;  // NaN fails every comparison
}

}  // namespace sp

using namespace sp;

extern "C" {

int64_t sp_prox_cg_workspace(const sp_op* op, int64_t batch, int32_t step_form) {
    if (!valid_op(op) || batch <= 0 || batch > 65535 || (step_form != 0 && step_form != 1))
        return SP_EINVAL;
    if (!cg_serves(op)) return SP_EUNSUPPORTED;
    return cg_plan(op, batch, step_form != 0, nullptr).floats;
}

int sp_op_prox_cg_ws(const sp_op* op, const float* x0, const float* y, int64_t batch, int64_t y_div,
                     float rho, int32_t max_iter, float tol, float* z_out, int32_t* iters_out,
                     float* work, sp_stream_t stream) {
    if (!valid_op(op) || !x0 || !y || !z_out || !work || batch <= 0 || y_div <= 0 ||
        batch > 65535 || !cg_scalars_ok(rho, max_iter, tol))
        return SP_EINVAL;
    if (!cg_serves(op)) return SP_EUNSUPPORTED;
    const cg_args a = {x0, nullptr, y, nullptr, 0, 0, 0, batch, y_div, {1.f, 1.f, rho, 0.f, 0.f, 0.f},
                       max_iter, tol, z_out, iters_out, work};
    return cg_run(op, a, static_cast<hipStream_t>(stream));
}

int sp_diffpir_step_cg_ws(const sp_op* op, const float* x, const float* eps, const float* y,
                          const float* xi, uint64_t seed, int64_t step, int64_t sample_offset,
                          int64_t batch, int64_t y_div, const sp_prox_coefs* coefs,
                          int32_t max_iter, float tol, float* x_out, int32_t* iters_out,
                          float* work, sp_stream_t stream) {
    if (!valid_op(op) || !x || !eps || !y || !coefs || !x_out || !work || batch <= 0 ||
        y_div <= 0 || batch > 65535 || !cg_scalars_ok(coefs->rho, max_iter, tol) || coefs->k == 0.f)
        return SP_EINVAL;
    if (!cg_serves(op)) return SP_EUNSUPPORTED;
    const cg_args a = {x, eps, y, xi, seed, step, sample_offset, batch, y_div, *coefs,
                       max_iter, tol, x_out, iters_out, work};
    return cg_run(op, a, static_cast<hipStream_t>(stream));
}

}  // extern "C"
