// x s super-resolution (SP_OP_SR): A = s x s average pooling of every channel plane,
// s in {2, 4, 8}.  A is block-diagonal over the s x s pixel blocks, so A^T, A^T A, A^+ = s^2 A^T
// and every residual, cotangent and AdamW term the samplers need are local to one block: each
// entry point that takes an sp_op is ONE pass over x with no halo (the reference has no such
// operator; semantics in operators/superres.py).
//
// Tile body (shared by all kernels below): a thread owns a patch of S rows x PW columns of one
// plane.  PW = 4 on the vector path (planes with W % 4 == 0: one float4 per patch row, all row
// loads issued before any arithmetic), so a patch is two blocks (S = 2), exactly one (S = 4) or
// the left / right half of one (S = 8: the two lanes of a pair exchange their half sums with
// __shfl_xor, no LDS).  Patches are numbered along the row (column group fastest, then the
// patch rows of all planes), consecutive lanes take consecutive patches, so one load
// instruction of a wave covers contiguous bytes of an image row.  W % 4 != 0 can only happen
// with S = 2 (factors 4 and 8 divide W); those planes take the scalar path PW = S = 2, one
// thread per low-resolution pixel.
//
// Arithmetic: 1 / s^2 is a power of two, so the scaling of A, A^T and A^+ is exact; only the
// s^2-term block sum rounds, and it is always taken in this order, whatever the path, batch or
// shard: within a patch row the lane's columns pairwise, (c0 + c1) [+ (c2 + c3)]; the S row
// sums by a balanced tree, ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); for S = 8 the
// left half plus the right half (one commutative add, so both lanes hold the same bits).
// Residual-norm partials: one per tile (block_sum's fixed order), grid = (tiles, batch).

#include <algorithm>

#define SP_TU 15  // debug-build site numbering (sp_common.h SP_DCHECK)
#include "sp_ops.h"

namespace sp {

template <int S, int PW>
struct sr_cfg {
    static_assert((S == 2 || S == 4 || S == 8) && (PW == 4 || (PW == 2 && S == 2)), "patch shape");
    static constexpr int NY = PW > S ? PW / S : 1;     // low-resolution pixels of a patch
    static constexpr bool kPair = PW < S;              // two lanes share one block (S = 8)
    static constexpr int kIter = (PW == 4 && S == 2) ? 2 : 1;  // patches per thread
    static constexpr int kTile = kBlock * kIter;       // patches per workgroup (even)
    static constexpr float kInv = 1.f / (S * S);
};

// where patch p of a sample lies: offset of its first element in the x row, of its first
// low-resolution pixel in the y row.  p counts (patch row over all planes, column group).
template <int S, int PW>
struct sr_patch {
    int64_t xo, yo;
    bool own;  // this lane writes / counts the patch's low-resolution pixel(s)
    __device__ __forceinline__ sr_patch(const sp_op& op, int64_t p) {
        const int wg = op.width / PW;  // column groups per row
        const int64_t row = p / wg;    // patch row: plane * (H / S) + row of blocks
        const int cg = static_cast<int>(p - row * wg);
        xo = row * S * op.width + cg * PW;
        yo = row * (op.width / S) + (cg * PW) / S;
        own = !sr_cfg<S, PW>::kPair || (cg & 1) == 0;
        SP_DCHECK(xo >= 0 && xo + (int64_t)(S - 1) * op.width + PW <= op.n);
        SP_DCHECK((yo >= 0 && yo + sr_cfg<S, PW>::NY <= op.m));
    }
};

template <int S, int PW, bool NT = false>
__device__ __forceinline__ void sr_load(const float* __restrict__ base, int64_t xo, int width,
                                        float (&r)[S][PW]) {
#pragma unroll
    for (int i = 0; i < S; ++i) {
        if constexpr (PW == 4) {
            load_v<4, NT>(base + xo + (int64_t)i * width, r[i]);
        } else {
#pragma unroll
            for (int e = 0; e < PW; ++e) r[i][e] = base[xo + (int64_t)i * width + e];
        }
    }
}

template <int S, int PW>
__device__ __forceinline__ void sr_store(float* __restrict__ base, int64_t xo, int width,
                                         const float (&r)[S][PW]) {
#pragma unroll
    for (int i = 0; i < S; ++i) {
        if constexpr (PW == 4) {
            store_v<4>(base + xo + (int64_t)i * width, r[i]);
        } else {
#pragma unroll
            for (int e = 0; e < PW; ++e) base[xo + (int64_t)i * width + e] = r[i][e];
        }
    }
}

// the patch's NY low-resolution pixels of a y row
template <int NY>
__device__ __forceinline__ void sr_load_y(const float* __restrict__ yb, int64_t yo, float (&y)[NY]) {
    if constexpr (NY == 2) {
        const float2 t = *reinterpret_cast<const float2*>(yb + yo);  // yo is even (W % 4 == 0)
        y[0] = t.x, y[1] = t.y;
    } else {
        y[0] = yb[yo];
    }
}

template <int NY>
__device__ __forceinline__ void sr_store_y(float* __restrict__ yb, int64_t yo, const float (&y)[NY]) {
    if constexpr (NY == 2) {
        *reinterpret_cast<float2*>(yb + yo) = make_float2(y[0], y[1]);
    } else {
        yb[yo] = y[0];
    }
}

// Block sums of a patch in the fixed order of the file comment.  Every lane of the wave must
// call it (S = 8 exchanges half sums between the lanes of a pair).
template <int S, int PW>
__device__ __forceinline__ void sr_block_sums(const float (&r)[S][PW], float (&sum)[sr_cfg<S, PW>::NY]) {
    constexpr int NY = sr_cfg<S, PW>::NY;
#pragma unroll
    for (int j = 0; j < NY; ++j) {
        float rows[S];
#pragma unroll
        for (int i = 0; i < S; ++i) {
            if constexpr (PW == 4 && S >= 4) rows[i] = (r[i][0] + r[i][1]) + (r[i][2] + r[i][3]);
            else rows[i] = r[i][2 * j] + r[i][2 * j + 1];
        }
#pragma unroll
        for (int w = 1; w < S; w *= 2)
#pragma unroll
            for (int i = 0; i < S; i += 2 * w) rows[i] += rows[i + w];
        sum[j] = rows[0];
    }
    if constexpr (sr_cfg<S, PW>::kPair) sum[0] += __shfl_xor(sum[0], 1, 64);
}

// column e of a patch belongs to low-resolution pixel e / S of the patch (0 when PW <= S)
template <int S, int PW>
__device__ __forceinline__ constexpr int sr_pixel_of(int e) { return PW > S ? e / S : 0; }

// y = A x
template <int S, int PW>
__global__ __launch_bounds__(kBlock) void k_sr_apply(sp_op op, const float* __restrict__ x,
                                                     float* __restrict__ y) {
    using cfg = sr_cfg<S, PW>;
    const int64_t b = blockIdx.y, T = op.n / (S * PW);
#pragma unroll
    for (int it = 0; it < cfg::kIter; ++it) {
        const int64_t p = (int64_t)blockIdx.x * cfg::kTile + it * kBlock + threadIdx.x;
        const bool in = p < T;  // pairs are in or out together (T and the tile base are even)
        float r[S][PW] = {};
        const sr_patch<S, PW> pt(op, in ? p : 0);
        if (in) sr_load<S, PW>(x + b * op.n, pt.xo, op.width, r);
        float s[cfg::NY];
        sr_block_sums<S, PW>(r, s);
#pragma unroll
        for (int j = 0; j < cfg::NY; ++j) s[j] *= cfg::kInv;
        if (in && pt.own) sr_store_y<cfg::NY>(y + b * op.m, pt.yo, s);
    }
}

// x = scale * (y replicated over its block): scale = 1 / s^2 is A^T
template <int S, int PW>
__global__ __launch_bounds__(kBlock) void k_sr_adjoint(sp_op op, const float* __restrict__ y,
                                                       float scale, float* __restrict__ x) {
    using cfg = sr_cfg<S, PW>;
    const int64_t b = blockIdx.y, T = op.n / (S * PW);
#pragma unroll
    for (int it = 0; it < cfg::kIter; ++it) {
        const int64_t p = (int64_t)blockIdx.x * cfg::kTile + it * kBlock + threadIdx.x;
        if (p >= T) continue;
        const sr_patch<S, PW> pt(op, p);
        float yv[cfg::NY], r[S][PW];
        sr_load_y<cfg::NY>(y + b * op.m, pt.yo, yv);
#pragma unroll
        for (int i = 0; i < S; ++i)
#pragma unroll
            for (int e = 0; e < PW; ++e) r[i][e] = scale * yv[sr_pixel_of<S, PW>(e)];
        sr_store<S, PW>(x + b * op.n, pt.xo, op.width, r);
    }
}

// DPS pass 1: x0 = (x - k eps) / a on the block, r = y - mean(x0), v = (gs / s^2) r broadcast,
// r^2 partial of the tile
template <int S, int PW>
__global__ __launch_bounds__(kBlock) void k_sr_dps_residual(sp_op op, const float* __restrict__ x,
                                                            const float* __restrict__ eps,
                                                            const float* __restrict__ y, int64_t y_div,
                                                            float a, float k, float gs,
                                                            float* __restrict__ v,
                                                            float* __restrict__ partial, int P,
                                                            const sp_step_rec* __restrict__ sched,
                                                            const int32_t* __restrict__ cursor) {
    using cfg = sr_cfg<S, PW>;
    __shared__ float red[4];
    if (sched) {  // device-resident schedule (graph replay): uniform scalar loads
        const sp_dps_coefs& c = sched[*cursor].c;
        a = c.a, k = c.k, gs = c.grad_scale;
    }
    const int64_t b = blockIdx.y, T = op.n / (S * PW);
    const float* yb = y + (b / y_div) * op.m;
    const float gsi = gs * cfg::kInv;
    float acc = 0.f;
#pragma unroll
    for (int it = 0; it < cfg::kIter; ++it) {
        const int64_t p = (int64_t)blockIdx.x * cfg::kTile + it * kBlock + threadIdx.x;
        const bool in = p < T;
        const sr_patch<S, PW> pt(op, in ? p : 0);
        // issue every load of the patch first (memory-level parallelism), then compute
        float xv[S][PW] = {}, ev[S][PW] = {}, yv[cfg::NY] = {};
        if (in) {
            sr_load<S, PW, true>(x + b * op.n, pt.xo, op.width, xv);
            sr_load<S, PW, true>(eps + b * op.n, pt.xo, op.width, ev);
            sr_load_y<cfg::NY>(yb, pt.yo, yv);
        }
#pragma unroll
        for (int i = 0; i < S; ++i)
#pragma unroll
            for (int e = 0; e < PW; ++e) xv[i][e] = (xv[i][e] - k * ev[i][e]) / a;
        float s[cfg::NY], vv[cfg::NY];
        sr_block_sums<S, PW>(xv, s);
#pragma unroll
        for (int j = 0; j < cfg::NY; ++j) {
            const float r = yv[j] - s[j] * cfg::kInv;
            vv[j] = gsi * r;
            if (in && pt.own) acc += r * r;
        }
        if (in) {
#pragma unroll
            for (int i = 0; i < S; ++i)
#pragma unroll
                for (int e = 0; e < PW; ++e) xv[i][e] = vv[sr_pixel_of<S, PW>(e)];
            sr_store<S, PW>(v + b * op.n, pt.xo, op.width, xv);
        }
    }
    const float t = block_sum(acc, red);
    SP_DCHECK(static_cast<int>(blockIdx.x) < P);
    if (threadIdx.x == 0) partial[b * P + blockIdx.x] = t;
}

// PSLD pixel pass: r = y - A x0, atr = A^T r, x_eff = x0 + atr (= A^T y + x0 - A^T A x0)
template <int S, int PW>
__global__ __launch_bounds__(kBlock) void k_sr_psld_pixel(sp_op op, const float* __restrict__ x0,
                                                          const float* __restrict__ y, int64_t y_div,
                                                          float* __restrict__ x_eff,
                                                          float* __restrict__ atr,
                                                          float* __restrict__ partial, int P) {
    using cfg = sr_cfg<S, PW>;
    __shared__ float red[4];
    const int64_t b = blockIdx.y, T = op.n / (S * PW);
    const float* yb = y + (b / y_div) * op.m;
    float acc = 0.f;
#pragma unroll
    for (int it = 0; it < cfg::kIter; ++it) {
        const int64_t p = (int64_t)blockIdx.x * cfg::kTile + it * kBlock + threadIdx.x;
        const bool in = p < T;
        const sr_patch<S, PW> pt(op, in ? p : 0);
        float xv[S][PW] = {}, yv[cfg::NY] = {};
        if (in) {
            sr_load<S, PW>(x0 + b * op.n, pt.xo, op.width, xv);
            sr_load_y<cfg::NY>(yb, pt.yo, yv);
        }
        float s[cfg::NY], ar[cfg::NY];
        sr_block_sums<S, PW>(xv, s);
#pragma unroll
        for (int j = 0; j < cfg::NY; ++j) {
            const float r = yv[j] - s[j] * cfg::kInv;
            ar[j] = r * cfg::kInv;
            if (in && pt.own) acc += r * r;
        }
        if (in) {
            float av[S][PW];
#pragma unroll
            for (int i = 0; i < S; ++i)
#pragma unroll
                for (int e = 0; e < PW; ++e) {
                    av[i][e] = ar[sr_pixel_of<S, PW>(e)];
                    xv[i][e] += av[i][e];
                }
            sr_store<S, PW>(atr + b * op.n, pt.xo, op.width, av);
            sr_store<S, PW>(x_eff + b * op.n, pt.xo, op.width, xv);
        }
    }
    const float t = block_sum(acc, red);
    SP_DCHECK(static_cast<int>(blockIdx.x) < P);
    if (threadIdx.x == 0) partial[b * P + blockIdx.x] = t;
}

// c_x0 = -omega atr / L + (I - A^T A) u, with A^T A u = (block mean of u) / s^2 broadcast
template <int S, int PW>
__global__ __launch_bounds__(kBlock) void k_sr_psld_cotangent(sp_op op, const float* __restrict__ atr,
                                                              const float* __restrict__ u,
                                                              const float* __restrict__ norm_sq,
                                                              float omega, float* __restrict__ out) {
    using cfg = sr_cfg<S, PW>;
    const float cl = -omega * inv_norm(norm_sq);
    const int64_t b = blockIdx.y, T = op.n / (S * PW);
#pragma unroll
    for (int it = 0; it < cfg::kIter; ++it) {
        const int64_t p = (int64_t)blockIdx.x * cfg::kTile + it * kBlock + threadIdx.x;
        const bool in = p < T;
        const sr_patch<S, PW> pt(op, in ? p : 0);
        float uv[S][PW] = {}, av[S][PW] = {};
        if (in) {
            sr_load<S, PW>(u + b * op.n, pt.xo, op.width, uv);
            sr_load<S, PW>(atr + b * op.n, pt.xo, op.width, av);
        }
        float s[cfg::NY];
        sr_block_sums<S, PW>(uv, s);
        if (in) {
#pragma unroll
            for (int i = 0; i < S; ++i)
#pragma unroll
                for (int e = 0; e < PW; ++e)
                    uv[i][e] = cl * av[i][e] +
                               (uv[i][e] - (s[sr_pixel_of<S, PW>(e)] * cfg::kInv) * cfg::kInv);
            sr_store<S, PW>(out + b * op.n, pt.xo, op.width, uv);
        }
    }
}

// One iteration of ReSample's pixel-space hard data consistency (sp_latent.hip k_pixel_opt):
// r = y - A x, g = A^T(gs r), AdamW update of x in place, r^2 partial of the loss before the
// update.  A set *stop makes it a no-op.
template <int S, int PW>
__global__ __launch_bounds__(kBlock) void k_sr_pixel_opt(sp_op op, float* __restrict__ x,
                                                         float* __restrict__ m, float* __restrict__ v,
                                                         const float* __restrict__ y, int64_t y_div,
                                                         float gs, sp_adamw_coefs c,
                                                         const int32_t* __restrict__ stop,
                                                         float* __restrict__ partial, int P) {
    using cfg = sr_cfg<S, PW>;
    __shared__ float red[4];
    if (stop && *stop) return;
    const int64_t b = blockIdx.y, T = op.n / (S * PW);
    const float* yb = y + (b / y_div) * op.m;
    const float gsi = gs * cfg::kInv;
    float acc = 0.f;
#pragma unroll
    for (int it = 0; it < cfg::kIter; ++it) {
        const int64_t p = (int64_t)blockIdx.x * cfg::kTile + it * kBlock + threadIdx.x;
        const bool in = p < T;
        const sr_patch<S, PW> pt(op, in ? p : 0);
        float xv[S][PW] = {}, mv[S][PW] = {}, vv[S][PW] = {}, yv[cfg::NY] = {};
        if (in) {
            sr_load<S, PW>(x + b * op.n, pt.xo, op.width, xv);
            sr_load<S, PW>(m + b * op.n, pt.xo, op.width, mv);
            sr_load<S, PW>(v + b * op.n, pt.xo, op.width, vv);
            sr_load_y<cfg::NY>(yb, pt.yo, yv);
        }
        float s[cfg::NY], g[cfg::NY];
        sr_block_sums<S, PW>(xv, s);
#pragma unroll
        for (int j = 0; j < cfg::NY; ++j) {
            const float r = yv[j] - s[j] * cfg::kInv;
            g[j] = gsi * r;
            if (in && pt.own) acc += r * r;
        }
        if (in) {
#pragma unroll
            for (int i = 0; i < S; ++i)
#pragma unroll
                for (int e = 0; e < PW; ++e)
                    adamw_1(xv[i][e], g[sr_pixel_of<S, PW>(e)], mv[i][e], vv[i][e], c);
            sr_store<S, PW>(x + b * op.n, pt.xo, op.width, xv);
            sr_store<S, PW>(m + b * op.n, pt.xo, op.width, mv);
            sr_store<S, PW>(v + b * op.n, pt.xo, op.width, vv);
        }
    }
    const float t = block_sum(acc, red);
    SP_DCHECK(static_cast<int>(blockIdx.x) < P);
    if (threadIdx.x == 0) partial[b * P + blockIdx.x] = t;
}

// xi of one patch row, PW elements from flat element index j of sample b: noise_v's forms.  A
// PW = 2 row starts at any even j, so its two elements are read or drawn one by one.
template <int PW, bool XI_IN>
__device__ __forceinline__ void sr_row_noise(const float* __restrict__ xi, uint64_t seed,
                                             int64_t step, int64_t sample_offset, int64_t b,
                                             int64_t n, int64_t j, float (&nz)[PW]) {
    if constexpr (PW == 4) {
        SP_DCHECK(j % 4 == 0);
        noise_v<4, XI_IN>(xi, seed, step, sample_offset, b, n, j, nz);
    } else {
        float q1[1];
        noise_v<1, XI_IN>(xi, seed, step, sample_offset, b, n, j, q1);
        nz[0] = q1[0];
        noise_v<1, XI_IN>(xi, seed, step, sample_offset, b, n, j + 1, q1);
        nz[1] = q1[0];
    }
}

// The proximal data step (A A^T = I / s^2): z = x0 + (r replicated over its block) / (1 + rho s^2)
// with r = y - (block mean of x0, summed in the file comment's order).  STEP false
// (sp_op_prox_ws): x holds x0, z is written.  STEP true (sp_diffpir_step_ws):
//   x0 = (x - k eps) / a,  eps_hat = (x - a z) / k,  x' = a_prev z + (c_eps eps_hat + c_xi xi)
// xi read, or drawn by Philox at the flat element index of every patch row (XI_IN false).  The
// divisions are multiplications by reciprocals taken once per thread; rho s^2 is exact.  A patch
// is read and written by its own lane alone, so the output may alias x.
template <int S, int PW, bool STEP, bool XI_IN>
__global__ __launch_bounds__(kBlock) void k_sr_prox(sp_op op, const float* __restrict__ x,
                                                    const float* __restrict__ eps,
                                                    const float* __restrict__ y,
                                                    const float* __restrict__ xi, uint64_t seed,
                                                    int64_t step, int64_t sample_offset,
                                                    int64_t y_div, sp_prox_coefs c,
                                                    float* __restrict__ out) {
    using cfg = sr_cfg<S, PW>;
    const int64_t b = blockIdx.y, T = op.n / (S * PW);
    const float* yb = y + (b / y_div) * op.m;
    const float inv_d = 1.f / (1.f + c.rho * static_cast<float>(S * S));
    const float inv_a = STEP ? 1.f / c.a : 1.f, inv_k = STEP ? 1.f / c.k : 1.f;
#pragma unroll
    for (int it = 0; it < cfg::kIter; ++it) {
        const int64_t p = (int64_t)blockIdx.x * cfg::kTile + it * kBlock + threadIdx.x;
        const bool in = p < T;  // pairs are in or out together (T and the tile base are even)
        const sr_patch<S, PW> pt(op, in ? p : 0);
        float xv[S][PW] = {}, zv[S][PW] = {}, yv[cfg::NY] = {};
        if (in) {
            sr_load<S, PW, true>(x + b * op.n, pt.xo, op.width, xv);
            if constexpr (STEP) sr_load<S, PW, true>(eps + b * op.n, pt.xo, op.width, zv);
            sr_load_y<cfg::NY>(yb, pt.yo, yv);
        }
        // every product and sum of the step rounds on its own (no contraction): the bits are those
        // of the expressions as written, whichever noise form the kernel was built for
#pragma unroll
        for (int i = 0; i < S; ++i)
#pragma unroll
            for (int e = 0; e < PW; ++e) {
#pragma clang fp contract(off)
                zv[i][e] = STEP ? (xv[i][e] - c.k * zv[i][e]) * inv_a : xv[i][e];  // x0
            }
        float s[cfg::NY], d[cfg::NY];
        sr_block_sums<S, PW>(zv, s);  // every lane of the wave: S = 8 exchanges half sums
#pragma unroll
        for (int j = 0; j < cfg::NY; ++j) {
#pragma clang fp contract(off)
            d[j] = (yv[j] - s[j] * cfg::kInv) * inv_d;
        }
        if (!in) continue;
#pragma unroll
        for (int i = 0; i < S; ++i) {
            float nz[PW] = {};
            if constexpr (STEP) {
                const int64_t j = pt.xo + (int64_t)i * op.width;  // flat element index of the row
                sr_row_noise<PW, XI_IN>(xi, seed, step, sample_offset, b, op.n, j, nz);
            }
#pragma unroll
            for (int e = 0; e < PW; ++e) {
#pragma clang fp contract(off)
                const float z = zv[i][e] + d[sr_pixel_of<S, PW>(e)];
                zv[i][e] = STEP ? diffpir_update(c, inv_k, xv[i][e], z, nz[e]) : z;
            }
        }
        sr_store<S, PW>(out + b * op.n, pt.xo, op.width, zv);
    }
}

// The DDRM step (A A^T = I / s^2: every singular value is 1 / s, Pi = A^T A s^2 is the block mean
// replicated), the projector form of samplers_hip.h in one launch next to k_sr_prox.  With
// x0 = (x - k eps) / a, f = ddrm_class_coefs(c, 1 / s^2, true) (fo; fu the unobserved set's; both
// taken once per launch on the host) and mean() the block mean (sums in the file comment's order,
// 1 / s^2 exact):
//   d  = (((f_th - 1) mean(x0) - (c1 sig_prev) mean(eps)) + (f_xi - eta sig_prev) mean(xi)) + f_y y
//   x' = a_prev (((x0 + (c1 sig_prev) eps) + (eta sig_prev) xi) + d)
// xi read, or drawn by Philox at the flat element index of every patch row.  A patch is read and
// written by its own lane alone, so the output may alias x.  Bytes per element: 12 (x, eps read,
// x' written) + 4 / s^2 (y), + 4 with xi injected.  Roundings of the longest path: x0 (4: 1 / a,
// k eps, the difference, the product), the block sum (log2 s^2), f_th - 1 (5: f_th as in k_ddrm
// and the difference) and its product (1), three sums of d (3), the sum with d (1), a_prev (1):
// 15 + log2 s^2.
template <int S, int PW, bool XI_IN>
__global__ __launch_bounds__(kBlock) void k_sr_ddrm(sp_op op, const float* __restrict__ x,
                                                    const float* __restrict__ eps,
                                                    const float* __restrict__ y,
                                                    const float* __restrict__ xi, uint64_t seed,
                                                    int64_t step, int64_t sample_offset,
                                                    int64_t y_div, sp_ddrm_coefs c, ddrm_f fo,
                                                    ddrm_f fu, float* __restrict__ out) {
    using cfg = sr_cfg<S, PW>;
    const int64_t b = blockIdx.y, T = op.n / (S * PW);
    const float* yb = y + (b / y_div) * op.m;
    const float inv_a = 1.f / c.a;
    const float g_th = fo.th - 1.f, g_xi = fo.xi - fu.xi;  // both round once
#pragma unroll
    for (int it = 0; it < cfg::kIter; ++it) {
        const int64_t p = (int64_t)blockIdx.x * cfg::kTile + it * kBlock + threadIdx.x;
        const bool in = p < T;  // pairs are in or out together (T and the tile base are even)
        const sr_patch<S, PW> pt(op, in ? p : 0);
        float xv[S][PW] = {}, ev[S][PW] = {}, nz[S][PW] = {}, yv[cfg::NY] = {};
        if (in) {
            sr_load<S, PW, true>(x + b * op.n, pt.xo, op.width, xv);
            sr_load<S, PW, true>(eps + b * op.n, pt.xo, op.width, ev);
            sr_load_y<cfg::NY>(yb, pt.yo, yv);
#pragma unroll
            for (int i = 0; i < S; ++i) {
                const int64_t j = pt.xo + (int64_t)i * op.width;  // flat element index of the row
                sr_row_noise<PW, XI_IN>(xi, seed, step, sample_offset, b, op.n, j, nz[i]);
            }
        }
        // every product and sum of the step rounds on its own (no contraction): the bits are those
        // of the expressions as written, whichever noise form the kernel was built for
#pragma unroll
        for (int i = 0; i < S; ++i)
#pragma unroll
            for (int e = 0; e < PW; ++e) {
#pragma clang fp contract(off)
                xv[i][e] = (xv[i][e] - c.k * ev[i][e]) * inv_a;  // x0
            }
        float s0[cfg::NY], se[cfg::NY], sx[cfg::NY], d[cfg::NY];
        sr_block_sums<S, PW>(xv, s0);  // every lane of the wave: S = 8 exchanges half sums
        sr_block_sums<S, PW>(ev, se);
        sr_block_sums<S, PW>(nz, sx);
#pragma unroll
        for (int j = 0; j < cfg::NY; ++j) {
#pragma clang fp contract(off)
            d[j] = ((g_th * (s0[j] * cfg::kInv) - fu.ep * (se[j] * cfg::kInv)) +
                    g_xi * (sx[j] * cfg::kInv)) +
                   fo.y * yv[j];
        }
        if (!in) continue;
#pragma unroll
        for (int i = 0; i < S; ++i)
#pragma unroll
            for (int e = 0; e < PW; ++e) {
#pragma clang fp contract(off)
                xv[i][e] = c.a_prev * (((xv[i][e] + fu.ep * ev[i][e]) + fu.xi * nz[i][e]) +
                                       d[sr_pixel_of<S, PW>(e)]);
            }
        sr_store<S, PW>(out + b * op.n, pt.xo, op.width, xv);
    }
}

// ---------------------------------------------------------------------------
// host side (called from the entry points in sp_dps.hip / sp_latent.hip; `op` is valid)
// ---------------------------------------------------------------------------
static inline bool sr_vec(const sp_op* op) { return op->width % 4 == 0; }

// patches per workgroup of the path `op` takes
static inline int64_t sr_tile(const sp_op* op) {
    if (!sr_vec(op)) return sr_cfg<2, 2>::kTile;
    return op->factor == 2 ? sr_cfg<2, 4>::kTile : op->factor == 4 ? sr_cfg<4, 4>::kTile
                                                                   : sr_cfg<8, 4>::kTile;
}

bool sr_valid(const sp_op* op) {
    return (op->factor == 2 || op->factor == 4 || op->factor == 8) && op->channels > 0 &&
           op->height > 0 && op->width > 0 &&
           (int64_t)op->channels * op->height * op->width == op->n &&
           op->height % op->factor == 0 && op->width % op->factor == 0 &&
           op->m * op->factor * op->factor == op->n;
}

// tiles per sample = r^2 partials per sample
int64_t sr_partials(const sp_op* op) {
    const int64_t patches = op->n / ((int64_t)op->factor * (sr_vec(op) ? 4 : 2));
    return (patches + sr_tile(op) - 1) / sr_tile(op);
}

// f(S, PW) for the operator's factor and path (W % 4 != 0 implies factor 2)
template <typename F>
static void sr_select(const sp_op* op, F&& f) {
    if (!sr_vec(op)) f(int_c<2>{}, int_c<2>{});
    else if (op->factor == 2) f(int_c<2>{}, int_c<4>{});
    else if (op->factor == 4) f(int_c<4>{}, int_c<4>{});
    else f(int_c<8>{}, int_c<4>{});
}

static dim3 sr_grid(const sp_op* op, int64_t batch) { return sample_grid(sr_partials(op), batch); }

// KERNEL<S, PW> over the operator's tiles (a template's name cannot be passed to a function)
#define SR_LAUNCH(KIND, WORK, KERNEL, ...)                                                    \
    sr_select(op, [&](auto S, auto PW) {                                                      \
        launch_w(KIND, WORK, KERNEL<S(), PW()>, sr_grid(op, batch), dim3(kBlock), s, __VA_ARGS__); \
    })

int sr_apply(const sp_op* op, const float* x, float* y, int64_t batch, hipStream_t s) {
    SR_LAUNCH(0, 0.0, k_sr_apply, *op, x, y);
    return check_launch("sp_op_apply");
}

int sr_adjoint(const sp_op* op, const float* y, float* x, int64_t batch, hipStream_t s) {
    const float scale = 1.f / static_cast<float>(op->factor * op->factor);
    SR_LAUNCH(0, 0.0, k_sr_adjoint, *op, y, scale, x);
    return check_launch("sp_op_adjoint");
}

int sr_dps_residual(const sp_op* op, const dps_residual_args& r, hipStream_t s) {
    const int P = static_cast<int>(sr_partials(op));
    const int64_t batch = r.batch;
    SR_LAUNCH(TK_DPS_RESIDUAL, (double)batch, k_sr_dps_residual, *op, r.x, r.eps, r.y, r.y_div, r.a, r.k,
              r.gs, r.v, r.partial, P, r.sched, r.cursor);
    return check_launch("sp_dps_residual");
}

int sr_psld_pixel(const sp_op* op, const float* x0, const float* y, int64_t batch, int64_t y_div,
                  float* x_eff, float* atr, float* partial, hipStream_t s) {
    const int P = static_cast<int>(sr_partials(op));
    SR_LAUNCH(0, 0.0, k_sr_psld_pixel, *op, x0, y, y_div, x_eff, atr, partial, P);
    return check_launch("sp_psld_pixel");
}

int sr_psld_cotangent(const sp_op* op, const float* atr, const float* u,
                      const float* /*ata_u: A^T A u is computed in the kernel*/, const float* norm_sq,
                      float omega, int64_t batch, float* out, hipStream_t s) {
    SR_LAUNCH(0, 0.0, k_sr_psld_cotangent, *op, atr, u, norm_sq, omega, out);
    return check_launch("sp_psld_cotangent");
}

int sr_pixel_opt(const sp_op* op, float* x, float* exp_avg, float* exp_avg_sq, const float* y,
                 int64_t batch, int64_t y_div, float gs, const sp_adamw_coefs* c,
                 const int32_t* stop, float* partial, hipStream_t s) {
    const int P = static_cast<int>(sr_partials(op));
    SR_LAUNCH(0, 0.0, k_sr_pixel_opt, *op, x, exp_avg, exp_avg_sq, y, y_div, gs, *c, stop, partial, P);
    return check_launch("sp_pixel_opt_step");
}

// one launch over the blocks, alone (p.eps null) or inside the DiffPIR step (xi read or drawn)
int sr_prox(const sp_op* op, const prox_args& p, hipStream_t s) {
    sr_select(op, [&](auto S, auto PW) {
        select_bool(p.eps, [&](auto step) {
            select_bool(p.xi, [&](auto xin) {  // the prox form has no noise: one kernel
                launch(0, k_sr_prox<S(), PW(), step(), step() && xin()>, sr_grid(op, p.batch),
                       dim3(kBlock), s, *op, p.x, p.eps, p.y, p.xi, p.seed, p.step, p.sample_offset,
                       p.y_div, p.c, p.out);
            });
        });
    });
    return check_launch(p.eps ? "sp_diffpir_step_ws" : "sp_op_prox_ws");
}

// the DDRM step: one launch over the blocks, xi read or drawn
int sr_ddrm(const sp_op* op, const ddrm_args& p, hipStream_t s) {
    const float g = 1.f / static_cast<float>(op->factor * op->factor);  // the squared singular value
    const ddrm_f fo = ddrm_class_coefs(p.c, g, true), fu = ddrm_class_coefs(p.c, g, false);
    sr_select(op, [&](auto S, auto PW) {
        select_bool(p.xi, [&](auto xin) {
            launch(0, k_sr_ddrm<S(), PW(), xin()>, sr_grid(op, p.batch), dim3(kBlock), s, *op, p.x,
                   p.eps, p.y, p.xi, p.seed, p.step, p.sample_offset, p.y_div, p.c, fo, fu, p.out);
        });
    });
    return check_launch("sp_ddrm_step_ws");
}

#undef SR_LAUNCH

}  // namespace sp
