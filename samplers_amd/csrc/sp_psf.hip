// Point-spread-function blur (SP_OP_PSF): a dense depthwise 2-D PSF h of (2R+1)^2 fp32 taps,
// 1 <= R <= 30, reflect padding, applied to every channel plane (the reference has no blur;
// semantics in operators/psf.py, pinned in fp64 by tests/psf_ops.py):
//   (A x)(i, j)   = sum_{u,v} h[u][v] x~(i + u - R, j + v - R)        correlation, no flip
//   (A^T y)(i, j) = sum_{py in M_H(i)} sum_{px in M_W(j)} U(py, px)
//   U(p, q)       = sum_{u,v} h[u][v] r0(p - (u - R), q - (v - R))    r0 = y, 0 off the image
//   M_N(j)        = {j} + {-j : 1 <= j <= R} + {2(N-1) - j : N-1-R <= j <= N-2}
//
// One workgroup owns a 32 x 64 output tile of one plane.  The tile plus its R halo is staged in
// LDS (one load per element, the source index computed at staging time; rows of 132 floats),
// the taps beside it, zero-padded to a multiple of the chunk width of 8.  A thread owns 8
// adjacent outputs of one row and slides over the patch row: per chunk of 8 tap columns it
// reads 8 new patch values (the other 8 of its 16-wide window are the previous chunk's) and 8
// taps (an LDS broadcast), four ds_read_b128, and issues 64 FMAs on registers.  Lanes are
// placed so that every 16-lane group of a ds_read_b128 covers the 64 banks once: the row
// stride is 4 banks (132 mod 64), a lane's 8-column run 8 banks, and the wave's four run
// columns take their 16 rows rotated by two, so lane l starts at bank 4 (l mod 16).
//
// Work follows the PSF's support: while the taps are staged, one ballot per tap row gives its
// first and last non-zero column, and every thread sweeps only the chunks that cover that span
// (a wave-uniform trip count; all-zero rows cost nothing).  Zero taps inside a chunk add +-0,
// so for finite inputs the result is the dense sum.  Every pixel's sum runs tap row by tap
// row, column by column, whatever the batch, y_div or shard.
//
// The adjoint is a gather with the same sweep.  A fold term is the correlation of a mirrored
// image with taps flipped on the other axis only: with s_T(g) = r0(-g),
// U(-i, q) = sum_u h[u] s_T(i + u - R), and with s_B(g) = r0(2(H-1) - g),
// U(2(H-1) - i, q) = sum_u h[u] s_B(i + u - R); the same per column.  So a tile runs one pass
// per (row mirror, column mirror) pair that can reach it: the patch is staged through the
// mirror (zeros off the image), the taps flipped on the axes that are NOT mirrored, and the
// pass's sums added under the masks of M_H / M_W.  A mirrored patch is zero beyond the
// mirrored border, so a fold pass sweeps only the tap rows / columns that can meet it (about
// half of them per mirrored axis).  Interior tiles run one pass, edge tiles two, corner tiles
// four (up to nine when H or W is within a tile of 2R + 1).  No atomics.
//
// DPS pass 1 is two launches: `residual` forms x0 = (x - k eps) / a while staging, computes
// A x0, writes g = grad_scale (y - A x0) to the caller's work buffer and one |r|^2 partial per
// tile (block_sum's fixed order); `adjoint` computes v = A^T g.

#include <algorithm>

#define SP_TU 16  // debug-build site numbering (sp_common.h SP_DCHECK)
#include "sp_ops.h"

namespace sp {

constexpr int PTH = 32, PTW = 64;  // output tile
constexpr int PNX = 8;             // adjacent outputs per thread
constexpr int PCV = 8;             // tap columns per chunk
constexpr int PPS = 132;           // patch row stride: >= PTW + 64 taps, and 4 banks mod 64
constexpr int PUN = 4;             // patch rows a thread stages per batch of loads
static_assert(PTH * (PTW / PNX) == kBlock && PTH == 32 && PTW == 64, "thread placement");

typedef float f4 __attribute__((ext_vector_type(4)));

enum { PSF_APPLY = 0, PSF_ADJOINT = 1, PSF_RESIDUAL = 2 };
enum { MIR_NONE = 0, MIR_LO = 1, MIR_HI = 2 };

// LDS layout for radius R (floats): patch rows x PPS, taps K x KP, K + 1 spans
struct psf_geom {
    int K, KP, rows;
    __host__ __device__ explicit psf_geom(int R)
        : K(2 * R + 1), KP((2 * R + 1 + PCV - 1) / PCV * PCV), rows(PTH + 2 * R) {}
    __host__ __device__ int floats() const { return rows * PPS + K * KP + K + 1; }
};

__device__ __forceinline__ int psf_reflect(int g, int L) {
    if (g < 0) g = -g;
    if (g >= L) g = 2 * (L - 1) - g;
    return g < 0 ? 0 : (g >= L ? L - 1 : g);  // past the padded extent: any valid pixel (unused)
}

__device__ __forceinline__ int psf_mirror(int g, int L, int mir) {
    return mir == MIR_NONE ? g : mir == MIR_LO ? -g : 2 * (L - 1) - g;
}

// one 16-byte LDS read, kept whole (the optimiser otherwise splits it into dword pairs)
__device__ __forceinline__ f4 lds4(const float* p) {
    f4 v = *reinterpret_cast<const f4*>(p);
    asm("" : "+v"(v));
    return v;
}

// taps -> LDS, flipped on the chosen axes, zero-padded to KP columns; wave w stages tap rows
// w, w + 4, ... (lane = column) and its ballot of the non-zero taps gives the row's span:
// first chunk column (a multiple of 4) and chunk count, packed lo | n << 16.  Rows outside
// [u_lo, u_hi] and columns outside [v_lo, v_hi] are known to meet only zeros: left out.
__device__ __forceinline__ void psf_stage_taps(const float* __restrict__ taps, float* T, int* sp,
                                               int R, const psf_geom& g, bool flip_y, bool flip_x,
                                               int u_lo, int u_hi, int v_lo, int v_hi) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long cols =
        (v_hi >= 63 ? ~0ull : (1ull << (v_hi + 1)) - 1ull) & ~((1ull << v_lo) - 1ull);
    const int vsrc = flip_x ? 2 * R - lane : lane;
    for (int u = wv; u < g.K; u += kBlock / 64) {
        float t = 0.f;
        if (lane < g.K) t = taps[(flip_y ? 2 * R - u : u) * g.K + vsrc];
        if (lane < g.KP) T[u * g.KP + lane] = t;
        unsigned long long m = __ballot(t != 0.f) & cols;
        if (u < u_lo || u > u_hi) m = 0ull;
        int lo = 0, n = 0;
        if (m) {
            const int c0 = __ffsll(static_cast<long long>(m)) - 1, c1 = 64 - __clzll(static_cast<long long>(m));
            lo = c0 & ~3;
            n = (c1 - lo + PCV - 1) / PCV;
            if (lo + n * PCV > g.KP) lo = g.KP - n * PCV;  // stay inside the padded row
            SP_DCHECK(lo >= 0 && (lo & 3) == 0 && lo <= c0 && lo + n * PCV >= c1 && lo + n * PCV <= g.KP);
        }
        if (lane == 0) sp[u] = lo | (n << 16);
    }
    if (threadIdx.x == 0) sp[g.K] = 0;  // the sweep reads one span ahead
}

// acc[e] += sum_i t[i] w[e + i], w = (a0, a1, b0, b1): tap by tap, so every output's sum is in
// tap order
__device__ __forceinline__ void psf_fma(const f4& a0, const f4& a1, const f4& b0, const f4& b1,
                                        const f4& t0, const f4& t1, float (&acc)[PNX]) {
    const float w[PNX + PCV] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w,
                                b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    const float t[PCV] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
    for (int i = 0; i < PCV; ++i)
#pragma unroll
        for (int e = 0; e < PNX; ++e) acc[e] = fmaf(t[i], w[e + i], acc[e]);
}

// acc[e] += sum_{u,v} T[u][v] Pt[ty + u][x0 + e + v] over the spans, in (u, v) order
__device__ __forceinline__ void psf_sweep(const float* Pt, const float* T, const int* sp,
                                          const psf_geom& g, int ty, int x0, float (&acc)[PNX]) {
    int ahead = sp[0];
    for (int u = 0; u < g.K; ++u) {
        const int s = __builtin_amdgcn_readfirstlane(ahead);
        ahead = sp[u + 1];
        const int lo = s & 0xffff, n = s >> 16;
        if (n == 0) continue;
        SP_DCHECK(ty + u < g.rows && x0 + lo + n * PCV + PNX <= PPS && lo + n * PCV <= g.KP);
        const float* p = Pt + (ty + u) * PPS + x0 + lo;
        const float* t = T + u * g.KP + lo;
        f4 a0 = lds4(p), a1 = lds4(p + 4);
        int c = 0;
        for (; c + 2 <= n; c += 2) {  // the window's upper half is the next chunk's lower half
            const f4 b0 = lds4(p + 8), b1 = lds4(p + 12);
            psf_fma(a0, a1, b0, b1, lds4(t), lds4(t + 4), acc);
            a0 = lds4(p + 16), a1 = lds4(p + 20);
            psf_fma(b0, b1, a0, a1, lds4(t + 8), lds4(t + 12), acc);
            p += 2 * PCV, t += 2 * PCV;
        }
        if (c < n) psf_fma(a0, a1, lds4(p + 8), lds4(p + 12), lds4(t), lds4(t + 4), acc);
    }
}

// Pt[i][j] = src(i, j) for j < PW (0 in the rest of the row), PUN rows' loads in flight
template <class F>
__device__ __forceinline__ void psf_stage_patch(float* Pt, int rows, int PW, F src) {
    const int sx = threadIdx.x & 63, sr = threadIdx.x >> 6;  // lane = column
    constexpr int NJ = (PPS + 63) / 64, RS = kBlock / 64;
    for (int i0 = sr; i0 < rows; i0 += RS * PUN) {
        float val[PUN][NJ];
#pragma unroll
        for (int a = 0; a < PUN; ++a)
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) {
                const int i = i0 + RS * a, j = sx + 64 * jj;
                val[a][jj] = (i < rows && j < PW) ? src(i, j) : 0.f;
            }
#pragma unroll
        for (int a = 0; a < PUN; ++a)
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) {
                const int i = i0 + RS * a, j = sx + 64 * jj;
                if (i < rows && j < PPS) Pt[i * PPS + j] = val[a][jj];
            }
    }
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void k_psf(sp_op op, const float* __restrict__ in,
                                                const float* __restrict__ eps,
                                                const float* __restrict__ y, int64_t y_div, float a,
                                                float k, float gs, float* __restrict__ out,
                                                float* __restrict__ partial, int P,
                                                const sp_step_rec* __restrict__ sched,
                                                const int32_t* __restrict__ cursor) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float red[4];
    if (MODE == PSF_RESIDUAL && sched) {  // device-resident schedule (graph replay)
        const sp_dps_coefs& cf = sched[*cursor].c;
        a = cf.a, k = cf.k, gs = cf.grad_scale;
    }
    const int R = op.radius, H = op.height, W = op.width, C = op.channels;
    const psf_geom g(R);
    float* Pt = smem;
    float* T = Pt + g.rows * PPS;
    int* sp = reinterpret_cast<int*>(T + g.K * g.KP);

    const int tilesW = (W + PTW - 1) / PTW, tilesH = (H + PTH - 1) / PTH, tiles = tilesW * tilesH;
    const int c = static_cast<int>(blockIdx.x) / tiles;
    const int tile = static_cast<int>(blockIdx.x) - c * tiles;
    const int64_t b = blockIdx.y;
    const int R0 = (tile / tilesW) * PTH, C0 = (tile % tilesW) * PTW;
    SP_DCHECK(c < C && R0 < H && C0 < W && static_cast<int>(blockIdx.x) < P);
    const int plane = H * W;  // < 2^31: in-plane offsets are 32-bit
    const int64_t poff = (b * C + c) * (int64_t)plane;
    const float* __restrict__ ip = in + poff;

    // sweep placement (file comment): wave = 16 rows x 4 runs, rows rotated by 2 per run column
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, cxl = lane >> 4;
    const int ty = 16 * (wv & 1) + (((lane & 15) - 2 * cxl) & 15);
    const int x0 = (4 * (wv >> 1) + cxl) * PNX;
    const int jy = R0 + ty, jx0 = C0 + x0;
    const int PW = PTW + 2 * R;  // staged columns that carry data; the rest of a row is zero

    float acc[PNX];
#pragma unroll
    for (int e = 0; e < PNX; ++e) acc[e] = 0.f;

    if constexpr (MODE != PSF_ADJOINT) {
        const float* __restrict__ ep = MODE == PSF_RESIDUAL ? eps + poff : nullptr;
        psf_stage_taps(op.taps, T, sp, R, g, false, false, 0, 2 * R, 0, 2 * R);
        psf_stage_patch(Pt, g.rows, PW, [&](int i, int j) {
            const int so = psf_reflect(R0 - R + i, H) * W + psf_reflect(C0 - R + j, W);
            SP_DCHECK(so >= 0 && so < plane);
            float val = ip[so];
            if constexpr (MODE == PSF_RESIDUAL) val = (val - k * ep[so]) / a;
            return val;
        });
        __syncthreads();
        psf_sweep(Pt, T, sp, g, ty, x0, acc);
    } else {
        const bool lo_y = R0 <= R, hi_y = R0 + PTH - 1 >= H - 1 - R;
        const bool lo_x = C0 <= R, hi_x = C0 + PTW - 1 >= W - 1 - R;
        for (int my = MIR_NONE; my <= MIR_HI; ++my) {
            if ((my == MIR_LO && !lo_y) || (my == MIR_HI && !hi_y)) continue;
            const bool row_ok = my == MIR_NONE || (my == MIR_LO ? (jy >= 1 && jy <= R)
                                                                 : (jy >= H - 1 - R && jy <= H - 2));
            // the mirrored patch is zero past the mirrored border: patch row ty + u holds data
            // only for u <= R - R0 (low mirror) or u >= H - R0 + R - PTH (high mirror)
            const int u_lo = my == MIR_HI ? max(0, H - R0 + R - PTH) : 0;
            const int u_hi = my == MIR_LO ? R - R0 : 2 * R;
            for (int mx = MIR_NONE; mx <= MIR_HI; ++mx) {
                if ((mx == MIR_LO && !lo_x) || (mx == MIR_HI && !hi_x)) continue;
                const int v_lo = mx == MIR_HI ? max(0, W - C0 + R - PTW) : 0;
                const int v_hi = mx == MIR_LO ? R - C0 : 2 * R;
                __syncthreads();  // the previous pass's sweep is done with the patch and the taps
                psf_stage_taps(op.taps, T, sp, R, g, my == MIR_NONE, mx == MIR_NONE, u_lo, u_hi, v_lo,
                               v_hi);
                psf_stage_patch(Pt, g.rows, PW, [&](int i, int j) {
                    const int gi = psf_mirror(R0 - R + i, H, my), gj = psf_mirror(C0 - R + j, W, mx);
                    if (gi < 0 || gi >= H || gj < 0 || gj >= W) return 0.f;
                    SP_DCHECK(gi * W + gj < plane);
                    return ip[gi * W + gj];
                });
                __syncthreads();
                float part[PNX];
#pragma unroll
                for (int e = 0; e < PNX; ++e) part[e] = 0.f;
                psf_sweep(Pt, T, sp, g, ty, x0, part);
#pragma unroll
                for (int e = 0; e < PNX; ++e) {
                    const int jx = jx0 + e;
                    const bool col_ok = mx == MIR_NONE || (mx == MIR_LO ? (jx >= 1 && jx <= R)
                                                                         : (jx >= W - 1 - R && jx <= W - 2));
                    if (row_ok && col_ok) acc[e] += part[e];
                }
            }
        }
    }

    // epilogue: the run's outputs (float4 pairs where the row allows, else element by element)
    const bool row_in = jy < H;
    const int o0 = jy * W + jx0;
    float* __restrict__ op_out = out + poff;
    const bool vec = (W & 3) == 0 && row_in && jx0 + PNX <= W &&
                     (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    float racc = 0.f;
    if constexpr (MODE == PSF_RESIDUAL) {
        const float* __restrict__ yp = y + ((b / y_div) * C + c) * (int64_t)plane;
        const bool yvec = vec && (reinterpret_cast<uintptr_t>(y) & 15) == 0;
        float yv[PNX];
#pragma unroll
        for (int e = 0; e < PNX; ++e) yv[e] = 0.f;
        if (yvec) {
            load_v<4>(yp + o0, reinterpret_cast<float(&)[4]>(yv[0]));
            load_v<4>(yp + o0 + 4, reinterpret_cast<float(&)[4]>(yv[4]));
        } else if (row_in) {
#pragma unroll
            for (int e = 0; e < PNX; ++e)
                if (jx0 + e < W) yv[e] = yp[o0 + e];
        }
#pragma unroll
        for (int e = 0; e < PNX; ++e) {
            const float r = yv[e] - acc[e];
            acc[e] = gs * r;
            if (row_in && jx0 + e < W) racc += r * r;
        }
    }
    if (vec) {
        SP_DCHECK(o0 >= 0 && o0 + PNX <= plane);
        store_v<4>(op_out + o0, reinterpret_cast<const float(&)[4]>(acc[0]));
        store_v<4>(op_out + o0 + 4, reinterpret_cast<const float(&)[4]>(acc[4]));
    } else if (row_in) {
#pragma unroll
        for (int e = 0; e < PNX; ++e)
            if (jx0 + e < W) {
                SP_DCHECK(o0 + e >= 0 && o0 + e < plane);
                op_out[o0 + e] = acc[e];
            }
    }
    if constexpr (MODE == PSF_RESIDUAL) {
        const float t = block_sum(racc, red);
        SP_DCHECK(static_cast<int>(blockIdx.x) < P);
        if (threadIdx.x == 0) partial[b * P + blockIdx.x] = t;
    }
}

// ---------------------------------------------------------------------------
// host side (called from the entry points in sp_dps.hip; `op` is valid)
// ---------------------------------------------------------------------------
bool psf_valid(const sp_op* op) {
    return op->taps && op->radius >= 1 && op->radius <= 30 && op->m == op->n && op->channels > 0 &&
           (int64_t)op->channels * op->height * op->width == op->n &&
           op->height > 2 * op->radius && op->width > 2 * op->radius;
}

// tiles per sample = workgroups per sample = r^2 partials per sample
int64_t psf_partials(const sp_op* op) {
    return (int64_t)op->channels * ((op->height + PTH - 1) / PTH) * ((op->width + PTW - 1) / PTW);
}

// floats of grad_scale * r between the residual and the adjoint launch
int64_t psf_workspace(const sp_op* op, int64_t batch) { return batch * op->m; }

static inline size_t psf_lds_bytes(const sp_op* op) { return sizeof(float) * psf_geom(op->radius).floats(); }

// out = A in (PSF_APPLY) or A^T in (PSF_ADJOINT): the kernel's plain map, no x0, no residual
template <int MODE>
static int psf_map(int kind, const char* what, const sp_op* op, const float* in, float* out,
                   int64_t batch, hipStream_t s) {
    const int64_t P = psf_partials(op);
    launch_w(kind, 0.0, k_psf<MODE>, sample_grid(P, batch), dim3(kBlock), psf_lds_bytes(op), s, *op, in,
             (const float*)nullptr, (const float*)nullptr, (int64_t)1, 1.f, 0.f, 0.f, out,
             (float*)nullptr, static_cast<int>(P), (const sp_step_rec*)nullptr, (const int32_t*)nullptr);
    return check_launch(what);
}

int psf_apply(const sp_op* op, const float* x, float* y, int64_t batch, hipStream_t s) {
    return psf_map<PSF_APPLY>(0, "sp_op_apply", op, x, y, batch, s);
}

int psf_adjoint(const sp_op* op, const float* y, float* x, int64_t batch, hipStream_t s) {
    return psf_map<PSF_ADJOINT>(0, "sp_op_adjoint", op, y, x, batch, s);
}

// residual (x, eps, y -> work = grad_scale r, partials), then adjoint (work -> v)
int psf_dps_residual(const sp_op* op, const dps_residual_args& r, hipStream_t s) {
    const int64_t P = psf_partials(op);
    launch_w(TK_DPS_RESIDUAL, (double)r.batch, k_psf<PSF_RESIDUAL>, sample_grid(P, r.batch), dim3(kBlock),
             psf_lds_bytes(op), s, *op, r.x, r.eps, r.y, r.y_div, r.a, r.k, r.gs, r.work, r.partial,
             static_cast<int>(P), r.sched, r.cursor);
    const int rc = check_launch("sp_dps_residual_ws");
    if (rc != SP_OK) return rc;
    return psf_map<PSF_ADJOINT>(TK_DPS_RESIDUAL, "sp_dps_residual_ws", op, r.work, r.v, r.batch, s);
}

}  // namespace sp
