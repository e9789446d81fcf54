// SP_OP_HADAMARD: compressed sensing on a scrambled Walsh-Hadamard transform, y = S H D x on every
// channel plane (samplers_hip.h): D the sign vector in taps, H the Sylvester matrix of order
// n_p = height * width = 2^k times n_p^(-1/2), S the kept coefficients of keep_bits / word_rank in
// ascending natural order.  A A^T = I_m, A^+ = A^T, and H is symmetric: the same butterflies serve
// both directions.
//
// One kernel, k_hd: a workgroup loads a tile of 2^p floats into LDS, runs the add/subtract levels
// over the tile-index bits [b0, p), optionally turns the finished coefficients into the adjoint's
// input in place (the "mid" step: mask, gather from y, residual or affine form) and runs the same
// levels again, and stores.  A tile is either one contiguous run (cb == p: b0 = 0, the low levels)
// or 2^(p - cb) rows of 2^cb columns, the rows 2^kLo floats apart (b0 = cb: the high levels).
//   planes of n_p <= 2^kLo   one launch per map and per fused pass: the tile is the plane
//   larger planes            low stage: chunks of 2^kLo floats, levels 0 .. kLo-1, source formed in
//                            the loads (d applied there) -> work; high stage: all 2^(k - kLo) high
//                            rows by a run of >= 32 columns, the remaining levels, the mid step and
//                            the adjoint's high levels without leaving LDS, in place in work; low
//                            stage again: work -> levels -> d, n_p^(-1/2), the pass's base -> out
// Levels 0 and 1 run in registers on the float4 a thread loads; the others in passes of up to four
// levels, a thread holding the 2^nb values of a group.  The LDS image pads 4 floats after every 64
// (hd_addr): the pass over bits 2..5 and the float4 rows then meet every bank once, and the passes
// from bit 5 up read consecutive floats in consecutive lanes.
//
// Every sum is an fp32 add or subtract, n_p^(-1/2) is applied once per transform (a power of two
// for even k), no atomics: the r^2 partials are one block_sum per mid tile, and a plane is computed
// by its own workgroups, so a sample's bits do not depend on the batch, y_div or the shard.
#define SP_TU 25
#include <cmath>

#include "sp_ops.h"

namespace sp {
namespace {

constexpr int kLo = 12;       // levels of the low stage: 2^12 floats, 17 KB of LDS with the padding
constexpr int kMinCols = 5;   // a high tile's run of columns: at least 32 floats, one 128-byte line

enum { HS_PLAIN, HS_PLAIN_D, HS_X0, HS_DDRM, HS_UNPACK };                 // what the loads form
enum { HM_NONE, HM_RES, HM_AFF, HM_PACK };                                // the mid step
enum { HD_PLAIN, HD_SCALE_D, HD_PROX, HD_DIFFPIR, HD_DDRM, HD_NONE };     // what the stores write

struct hd_args {
    sp_op op;
    int p, cb, tiles;  // tile: 2^p floats, rows of 2^cb; tiles per plane
    int64_t np, mp;    // floats of a plane of x and of y
    float scale;       // n_p^(-1/2)
    const float *in, *eps, *xi, *y;  // in: rows of n (x, x0 or work); y: rows of m
    const float* x;                  // rows of n the stores read again (x, or x0 in the prox form)
    float *out, *yout, *partial;     // out: rows of n; yout: rows of m (HM_PACK)
    int64_t y_div, ystride;          // floats between the rows of y: m, or n for the q of sp_pgdm_prepare
    float a, k, g;                   // x0 = (x - k eps) / a; g: gs, 1 / (1 + rho) or f_y
    float w_th, w_ep, w_xi;          // DDRM: w = (w_th x0 + w_ep eps) + w_xi xi
    float b_ep, b_xi, a_prev;        //       x' = a_prev ((x0 + (b_ep eps + b_xi xi)) + A^T(..))
    sp_prox_coefs pc;
    uint64_t seed;
    int64_t step, sample_offset;
    const sp_step_rec* sched;
    const int32_t* cursor;
};

__device__ __forceinline__ int hd_addr(int e) { return e + ((e >> 6) << 2); }
inline size_t hd_lds_bytes(int p) { return sizeof(float) * ((size_t(1) << p) + (size_t(1) << p) / 16); }

// one pass: the levels of bits [b, b + NB) on every group of 2^NB values 2^b apart
template <int NB>
__device__ __forceinline__ void hd_pass(float* lds, int T, int b) {
    constexpr int R = 1 << NB;
    const int groups = T >> NB;
    for (int gi = threadIdx.x; gi < groups; gi += kBlock) {
        const int base = ((gi >> b) << (b + NB)) | (gi & ((1 << b) - 1));
        float v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            SP_DCHECK(base + (r << b) < T);
            v[r] = lds[hd_addr(base + (r << b))];
        }
#pragma unroll
        for (int h = 1; h < R; h <<= 1) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (!(r & h)) {
                    const float lo = v[r], hi = v[r | h];
                    v[r] = lo + hi;
                    v[r | h] = lo - hi;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) lds[hd_addr(base + (r << b))] = v[r];
    }
}

// the levels of bits [max(b0, 2), p) of the tile in LDS; a barrier before every pass and at the end
__device__ __forceinline__ void hd_levels(float* lds, int p, int b0) {
    const int T = 1 << p;
    for (int b = b0 < 2 ? 2 : b0; b < p; b += 4) {
        __syncthreads();
        const int nb = p - b < 4 ? p - b : 4;
        if (nb == 4) hd_pass<4>(lds, T, b);
        else if (nb == 3) hd_pass<3>(lds, T, b);
        else if (nb == 2) hd_pass<2>(lds, T, b);
        else hd_pass<1>(lds, T, b);
    }
    __syncthreads();
}

__device__ __forceinline__ void hd_x0(const float (&x)[4], const float (&e)[4], float a, float k,
                                      float (&o)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma clang fp contract(off)
        o[i] = (x[i] - k * e[i]) / a;
    }
}

template <int SRC, int MID, int DST>
__global__ __launch_bounds__(kBlock) void k_hd(hd_args g) {
    extern __shared__ __attribute__((aligned(16))) float hd_lds[];
    __shared__ float red4[4];
    float* lds = hd_lds;
    const int T = 1 << g.p, cmask = (1 << g.cb) - 1, b0 = g.cb == g.p ? 0 : g.cb;
    const int64_t plane = blockIdx.x / g.tiles;
    const int tile = static_cast<int>(blockIdx.x - plane * g.tiles);
    const int64_t b = plane / g.op.channels;
    const int c = static_cast<int>(plane - b * g.op.channels);
    const int64_t col0 = (int64_t)tile << g.cb;
    const int64_t poff = b * g.op.n + (int64_t)c * g.np;                      // the plane in rows of n
    const int64_t yoff = (b / g.y_div) * g.ystride + (int64_t)c * g.mp;         // and in the rows of y
    const float* d = g.op.taps;  // null: all +1
    if (g.sched) {  // device-resident schedule (graph replay)
        const sp_dps_coefs& cf = g.sched[*g.cursor].c;
        g.a = cf.a, g.k = cf.k, g.g = cf.grad_scale;
    }
    // plane index of tile element e (a multiple of 4 stays inside one row: cb >= 5)
    auto at = [&](int e) -> int64_t { return ((int64_t)(e >> g.cb) << kLo) + col0 + (e & cmask); };
    auto noise = [&](int64_t j, float (&z)[4]) {
        if (g.xi) load_v<4>(g.xi + poff + j, z);
        else philox_normals<4>(g.seed, g.step, g.sample_offset + b, (int64_t)c * g.np + j, z);
    };

    // ---- loads ----
    for (int e = 4 * threadIdx.x; e < T; e += 4 * kBlock) {
        const int64_t j = at(e);
        SP_DCHECK(j + 3 < g.np);
        float v[4];
        if constexpr (SRC == HS_UNPACK) {
            uint32_t bits;
            int64_t r;
            inpaint_lookup(g.op, j, bits, r);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[i] = 0.f;
                if ((bits >> i) & 1u) {
                    SP_DCHECK(r < g.mp);
                    v[i] = g.y[yoff + r];
                }
                r += (bits >> i) & 1u;
            }
        } else {
            load_v<4>(g.in + poff + j, v);
            if constexpr (SRC == HS_X0 || SRC == HS_DDRM) {
                float ev[4], x0[4];
                load_v<4>(g.eps + poff + j, ev);
                hd_x0(v, ev, g.a, g.k, x0);
                if constexpr (SRC == HS_DDRM) {
                    float z[4];
                    noise(j, z);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
#pragma clang fp contract(off)
                        v[i] = (g.w_th * x0[i] + g.w_ep * ev[i]) + g.w_xi * z[i];
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = x0[i];
                }
            }
            if constexpr (SRC != HS_PLAIN) {
                if (d) {
                    float dv[4];
                    load_v<4>(d + j, dv);
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = dv[i] * v[i];
                }
            }
        }
        if (b0 == 0) {  // levels 0 and 1 in registers
            const float s0 = v[0] + v[1], d0 = v[0] - v[1], s1 = v[2] + v[3], d1 = v[2] - v[3];
            v[0] = s0 + s1, v[1] = d0 + d1, v[2] = s0 - s1, v[3] = d0 - d1;
        }
        SP_DCHECK(hd_addr(e) + 3 < T + T / 16);
        store_v<4>(&lds[hd_addr(e)], v);
    }
    hd_levels(lds, g.p, b0);

    // ---- the finished coefficients -> the adjoint's input, in place ----
    if constexpr (MID != HM_NONE) {
        float rsq = 0.f;
        for (int e = 4 * threadIdx.x; e < T; e += 4 * kBlock) {
            const int64_t j = at(e);
            float v[4];
            load_v<4>(&lds[hd_addr(e)], v);
            uint32_t bits;
            int64_t r;
            inpaint_lookup(g.op, j, bits, r);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma clang fp contract(off)
                const float cf = g.scale * v[i];
                float u = 0.f;
                if ((bits >> i) & 1u) {
                    SP_DCHECK(r < g.mp);
                    if constexpr (MID == HM_PACK) {
                        g.yout[b * g.op.m + (int64_t)c * g.mp + r] = cf;
                    } else if constexpr (MID == HM_RES) {
                        const float rr = g.y[yoff + r] - cf;
                        rsq += rr * rr;
                        u = g.g * rr;
                    } else {
                        u = g.g * g.y[yoff + r] + cf;
                    }
                }
                r += (bits >> i) & 1u;
                v[i] = u;
            }
            if constexpr (MID != HM_PACK) store_v<4>(&lds[hd_addr(e)], v);
        }
        if constexpr (MID == HM_RES) {
            if (g.partial) {
                const float tot = block_sum(rsq, red4);
                if (threadIdx.x == 0)
                    g.partial[(b * g.op.channels + c) * (int64_t)g.tiles + tile] = tot;
            }
        }
        if constexpr (MID != HM_PACK) hd_levels(lds, g.p, b0);
    }

    // ---- stores ----
    if constexpr (DST != HD_NONE) {
        const float inv_k = DST == HD_DIFFPIR ? 1.f / g.pc.k : 1.f;
        for (int e = 4 * threadIdx.x; e < T; e += 4 * kBlock) {
            const int64_t j = at(e);
            float v[4];
            load_v<4>(&lds[hd_addr(e)], v);
            if (b0 == 0 && MID != HM_NONE) {  // the second transform's levels 0 and 1
                const float s0 = v[0] + v[1], d0 = v[0] - v[1], s1 = v[2] + v[3], d1 = v[2] - v[3];
                v[0] = s0 + s1, v[1] = d0 + d1, v[2] = s0 - s1, v[3] = d0 - d1;
            }
            if constexpr (DST != HD_PLAIN) {
                float dv[4] = {1.f, 1.f, 1.f, 1.f};
                if (d) load_v<4>(d + j, dv);
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = dv[i] * (g.scale * v[i]);
            }
            if constexpr (DST == HD_PROX) {
                float xv[4];
                load_v<4>(g.x + poff + j, xv);  // x0 itself: the prox form has no eps
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = xv[i] + v[i];
            } else if constexpr (DST == HD_DIFFPIR || DST == HD_DDRM) {
                float xv[4], ev[4], x0[4], z[4];
                load_v<4>(g.x + poff + j, xv);
                load_v<4>(g.eps + poff + j, ev);
                hd_x0(xv, ev, g.a, g.k, x0);
                noise(j, z);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma clang fp contract(off)
                    if constexpr (DST == HD_DIFFPIR)
                        v[i] = diffpir_update(g.pc, inv_k, xv[i], x0[i] + v[i], z[i]);
                    else
                        v[i] = g.a_prev * ((x0[i] + (g.b_ep * ev[i] + g.b_xi * z[i])) + v[i]);
                }
            }
            SP_DCHECK(j + 3 < g.np);
            store_v<4>(g.out + poff + j, v);
        }
    }
}

struct hd_geom {
    int k, hp, hcb;  // log2 n_p; the high tile: 2^hp floats, rows of 2^hcb
    bool split;
    int64_t np, mp;
    float scale;
};

int hd_log2(int64_t v) {
    int k = 0;
    while ((int64_t(1) << k) < v) ++k;
    return k;
}

hd_geom hd_geom_of(const sp_op* op) {
    hd_geom g;
    g.np = (int64_t)op->height * op->width, g.mp = op->m / op->channels;
    g.k = hd_log2(g.np);
    g.split = g.k > kLo;
    const int hb = g.k - kLo;  // the high levels
    g.hp = hb + kMinCols > kLo ? hb + kMinCols : kLo;
    g.hcb = g.hp - hb;
    // 2^(-k/2): a power of two for even k, its fp32 rounding for odd k
    g.scale = g.k % 2 == 0 ? std::ldexp(1.f, -g.k / 2) : static_cast<float>(std::exp2(-0.5 * g.k));
    return g;
}

enum { HT_PLANE, HT_CHUNK, HT_HIGH };

template <int SRC, int MID, int DST>
void hd_run(const sp_op* op, const hd_geom& g, int shape, hd_args a, int64_t batch, hipStream_t s) {
    a.op = *op, a.np = g.np, a.mp = g.mp, a.scale = g.scale;
    if (shape == HT_PLANE) a.p = a.cb = g.k, a.tiles = 1;
    else if (shape == HT_CHUNK) a.p = a.cb = kLo, a.tiles = static_cast<int>(g.np >> kLo);
    else a.p = g.hp, a.cb = g.hcb, a.tiles = 1 << (kLo - g.hcb);
    if (!a.y_div) a.y_div = 1;
    if (!a.ystride) a.ystride = op->m;
    const int64_t blocks = batch * op->channels * a.tiles;
    launch_w(0, 0.0, k_hd<SRC, MID, DST>, dim3(static_cast<unsigned>(blocks)), dim3(kBlock),
             hd_lds_bytes(a.p), s, a);
}

bool hd_grid_ok(const sp_op* op, int64_t batch) {
    return batch * op->channels * (((int64_t)op->height * op->width + 4095) >> kLo) <= 0x7fffffff;
}

// out = DST(A^T MID(A SRC(in))): one launch on a small plane, three through work on a larger one
template <int SRC, int MID, int DST>
void hd_fused(const sp_op* op, const hd_args& a, float* work, int64_t batch, hipStream_t s) {
    const hd_geom g = hd_geom_of(op);
    if (!g.split) return hd_run<SRC, MID, DST>(op, g, HT_PLANE, a, batch, s);
    hd_args l = a, h = a, f = a;
    l.out = work;
    hd_run<SRC, HM_NONE, HD_PLAIN>(op, g, HT_CHUNK, l, batch, s);
    h.in = work, h.out = work;
    hd_run<HS_PLAIN, MID, HD_PLAIN>(op, g, HT_HIGH, h, batch, s);
    f.in = work, f.partial = nullptr;
    hd_run<HS_PLAIN, HM_NONE, DST>(op, g, HT_CHUNK, f, batch, s);
}

int hd_forward(const sp_op* op, const float* x, float* y, int64_t batch, float* work, hipStream_t s) {
    if (!hd_grid_ok(op, batch)) return SP_EINVAL;
    const hd_geom g = hd_geom_of(op);
    hd_args a = {};
    a.in = x, a.yout = y;
    if (!g.split) {
        hd_run<HS_PLAIN_D, HM_PACK, HD_NONE>(op, g, HT_PLANE, a, batch, s);
    } else {
        hd_args l = a;
        l.out = work;
        hd_run<HS_PLAIN_D, HM_NONE, HD_PLAIN>(op, g, HT_CHUNK, l, batch, s);
        a.in = work;
        hd_run<HS_PLAIN, HM_PACK, HD_NONE>(op, g, HT_HIGH, a, batch, s);
    }
    return check_launch("hadamard forward");
}

int hd_backward(const sp_op* op, const float* y, float* x, int64_t batch, float* work, hipStream_t s) {
    if (!hd_grid_ok(op, batch)) return SP_EINVAL;
    const hd_geom g = hd_geom_of(op);
    hd_args a = {};
    a.y = y, a.out = x;
    if (!g.split) {
        hd_run<HS_UNPACK, HM_NONE, HD_SCALE_D>(op, g, HT_PLANE, a, batch, s);
    } else {
        hd_args h = a;
        h.out = work;
        hd_run<HS_UNPACK, HM_NONE, HD_PLAIN>(op, g, HT_HIGH, h, batch, s);
        a.in = work;
        hd_run<HS_PLAIN, HM_NONE, HD_SCALE_D>(op, g, HT_CHUNK, a, batch, s);
    }
    return check_launch("hadamard backward");
}

}  // namespace

bool hadamard_valid(const sp_op* op) {
    if (!op->keep_bits || !op->word_rank || op->channels < 1 || op->height < 1 || op->width < 1 ||
        op->radius != 0 || op->factor != 0)
        return false;
    const int64_t np = (int64_t)op->height * op->width;
    if ((np & (np - 1)) != 0 || np < 64 || np > (int64_t(1) << 20)) return false;
    if (op->n != op->channels * np || op->m % op->channels != 0) return false;
    const int64_t mp = op->m / op->channels;
    return mp >= 1 && mp <= np;
}

// one r^2 partial per mid tile: the plane, or the tiles of the high stage
int64_t hadamard_partials(const sp_op* op) {
    const hd_geom g = hd_geom_of(op);
    return (int64_t)op->channels * (g.split ? 1 << (kLo - g.hcb) : 1);
}

int64_t hadamard_workspace(const sp_op* op, int64_t batch) { return batch * op->n; }

int hadamard_apply(const sp_op* op, const float* x, float* y, int64_t batch, float* work, hipStream_t s) {
    return hd_forward(op, x, y, batch, work, s);
}

int hadamard_vjp(const sp_op* op, const float*, const float* gy, float* dx, int64_t batch, float* work,
                 hipStream_t s) {
    return hd_backward(op, gy, dx, batch, work, s);
}

// A^+ = A^T and A^+T = A
int hadamard_pinv(const sp_op* op, const float* y, float* x, int64_t batch, int transpose, float* work,
                  hipStream_t s) {
    return transpose ? hd_forward(op, y, x, batch, work, s) : hd_backward(op, y, x, batch, work, s);
}

// q is y itself, a row every n floats (sp_op_workspace of one sample), m of them used
int hadamard_pgdm_prepare(const sp_op* op, const float* y, int64_t rows, float* q, hipStream_t s) {
    const hipError_t e = hipMemcpy2DAsync(q, sizeof(float) * op->n, y, sizeof(float) * op->m,
                                          sizeof(float) * op->m, rows, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) set_error("sp_pgdm_prepare (hadamard)", e);
    return e == hipSuccess ? check_launch("sp_pgdm_prepare (hadamard)") : SP_ELAUNCH;
}

int hadamard_dps_residual(const sp_op* op, const dps_residual_args& r, hipStream_t s) {
    if (!hd_grid_ok(op, r.batch)) return SP_EINVAL;
    hd_args a = {};
    a.in = r.x, a.eps = r.eps, a.y = r.y, a.out = r.v, a.partial = r.partial, a.y_div = r.y_div;
    a.a = r.a, a.k = r.k, a.g = r.gs, a.sched = r.sched, a.cursor = r.cursor;
    hd_fused<HS_X0, HM_RES, HD_SCALE_D>(op, a, r.work, r.batch, s);
    return check_launch("sp_dps_residual (hadamard)");
}

int hadamard_pgdm_residual(const sp_op* op, const float* x, const float* eps, const float* q, int64_t batch,
                           int64_t y_div, const sp_dps_coefs& c, float* v, float* work, hipStream_t s) {
    if (!hd_grid_ok(op, batch)) return SP_EINVAL;
    hd_args a = {};
    a.in = x, a.eps = eps, a.y = q, a.out = v, a.y_div = y_div, a.ystride = op->n;
    a.a = c.a, a.k = c.k, a.g = c.grad_scale;
    hd_fused<HS_X0, HM_RES, HD_SCALE_D>(op, a, work, batch, s);
    return check_launch("sp_pgdm_residual_ws (hadamard)");
}

// both forms: p.eps selects the whole DiffPIR step.  z = x0 + A^T (y - A x0) / (1 + rho)
int hadamard_prox(const sp_op* op, const prox_args& p, hipStream_t s) {
    if (!p.work || !hd_grid_ok(op, p.batch)) return SP_EINVAL;
    hd_args a = {};
    a.in = a.x = p.x, a.y = p.y, a.out = p.out, a.y_div = p.y_div;
    a.g = 1.f / (1.f + p.c.rho);
    if (p.eps) {
        a.eps = p.eps, a.a = p.c.a, a.k = p.c.k, a.pc = p.c;
        a.xi = p.xi, a.seed = p.seed, a.step = p.step, a.sample_offset = p.sample_offset;
        hd_fused<HS_X0, HM_RES, HD_DIFFPIR>(op, a, p.work, p.batch, s);
    } else {
        hd_fused<HS_PLAIN_D, HM_RES, HD_PROX>(op, a, p.work, p.batch, s);
    }
    return check_launch(p.eps ? "sp_diffpir_step_ws (hadamard)" : "sp_op_prox_ws (hadamard)");
}

// x' = a_prev [base + A^T (f_y y + A w)]: the projector form of the spectral step, one class (s^2 = 1)
// for the whole kept set; q is y (sp_pgdm_prepare)
int hadamard_ddrm(const sp_op* op, const ddrm_args& p, hipStream_t s) {
    if (!hd_grid_ok(op, p.batch)) return SP_EINVAL;
    const ddrm_f fo = ddrm_class_coefs(p.c, 1.f, true), fu = ddrm_class_coefs(p.c, 1.f, false);
    hd_args a = {};
    a.in = a.x = p.x, a.eps = p.eps, a.y = p.q, a.out = p.out, a.y_div = p.y_div, a.ystride = op->n;
    a.xi = p.xi, a.seed = p.seed, a.step = p.step, a.sample_offset = p.sample_offset;
    a.a = p.c.a, a.k = p.c.k, a.g = fo.y, a.a_prev = p.c.a_prev;
    a.w_th = fo.th - fu.th, a.w_ep = fo.ep - fu.ep, a.w_xi = fo.xi - fu.xi;
    a.b_ep = fu.ep, a.b_xi = fu.xi;
    hd_fused<HS_DDRM, HM_AFF, HD_DDRM>(op, a, p.work, p.batch, s);
    return check_launch("sp_ddrm_step_ws (hadamard)");
}

}  // namespace sp
