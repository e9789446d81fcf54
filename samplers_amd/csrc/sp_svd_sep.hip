// SP_OP_SVD_SEPARABLE: A X = A_H X A_W^T on every channel plane, given by the SVDs of its two 1-D
// factors (samplers_hip.h: the tables V_H, V_W, U_H, U_W, S, P).  With T(X) = V_H^T X V_W (the
// forward transform, observed grid = its top-left Hy x Wy block) and T_y(Y) = U_H^T Y U_W every
// pass is a chain of per-plane dense products, one launch per side, the intermediate in the
// caller's workspace; the spectral arithmetic of a pass sits in the epilogue of the launch that
// produces the spectrum and x0 = (x - k eps) / a in the loads of the first one.
//
// One kernel, k_ss_gemm: D (M x N) = A (M x K) B (K x N) per plane on v_mfma_f32_32x32x2_f32
// (exact fp32: a chain of fmaf).  Both operands are (pointer, row stride, column stride), so the
// table stands on the left or on the right, plain or transposed, from its one row-major copy.  A
// workgroup of 4 waves owns a 64 x 64 tile of D (a wave a 32 x 32 quarter), walks K in chunks of
// 16 through two LDS tiles [16][64 (+4)], filled with zeros past the edges (padding adds exactly
// nothing), and masks its stores.  The tiling depends on the plane's sizes alone and a plane is
// computed by its own workgroups: the bits of a sample do not depend on the batch, y_div or shard.
// No atomics; the |r|^2 partials are one block_sum per tile.
//
// Work buffers: W0, W1, ... are batch * n floats each, a plane every H * W floats whatever the
// intermediate's size.  Launch sequences (L: table on the left, R: on the right):
//   A x / A^+T x   L V_H[:, :Hy]^T x -> W0; R W0 V_W[:, :Wy], times S (P) -> W1; L U_H W1 -> W0;
//                  R W0 U_W^T -> y
//   A^T g / A^+ y  L U_H^T g -> W0; R W0 U_W, times S (P) -> W1; L V_H[:, :Hy] W1 -> W0;
//                  R W0 V_W[:, :Wy]^T -> x
//   prepare        q has a row every 2 n floats (sp_op_workspace of one sample): L U_H^T y -> the
//                  row's floats [m, 2 m); R of that with U_W, times P (pgdm) or S (prox) -> [0, m)
//   DPS pass 1     the two prepare launches of y's rows -> W2 (no multiplier); L of x0 -> W0;
//                  R W0 V_W[:, :Wy] with g = gs S (yhat - S d) and one r^2 partial per tile -> W1;
//                  the last two launches of A^T
//   PGDM pass 1    L of x0 -> W0; R with gs (q - (P != 0 ? d : 0)) -> W1; the last two of A^T
//   prox / DiffPIR L V_H^T x0 (full H x W) -> W0; R W0 V_W with (q + rho d) / (S^2 + rho) on the
//                  observed grid and d elsewhere (a select) -> W1; L V_H W1 -> W0; R W0 V_W^T with
//                  diffpir_update in the epilogue (xi read, or drawn per tile into LDS) -> out
//   DDRM           L V_H^T of x0, eps and xi (read, or drawn by Philox in the loads) in one launch
//                  -> W0, W1, W2; R of the three with F = f_y q + f_th d0 + f_eps d1 + f_xi d2 -> W3;
//                  L V_H W3 -> W0; R W0 V_W^T times a_prev -> out
#define SP_TU 24
#include "sp_ops.h"

namespace sp {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kTile = 64, kChunk = 16, kLd = kTile + 4;  // LDS rows 16-byte aligned, 68 floats

enum { SS_SRC_PLAIN, SS_SRC_X0, SS_SRC_DDRM };
enum { SS_STORE, SS_MUL, SS_SCALE, SS_DPS, SS_PGDM, SS_PROX, SS_DIFFPIR, SS_DDRM };

struct ss_mat {
    const float* p;
    int64_t sample, plane;  // floats between samples and between a sample's planes, 0 for a table
    int64_t rs, cs;
    int64_t lim;    // floats of one plane the operand may touch (SP_DCHECK)
};

struct ss_gemm {
    ss_mat A, B;
    int M, N, K;
    float* out;
    int64_t o_sample, o_plane;
    int ldo;
    int C;               // planes per sample
    int64_t src_stride;  // DDRM: floats between the three transformed sources (out of L, A of R)
};

struct ss_pro {  // the loads of B: x0 from (x, eps), or the three DDRM sources
    const float *eps, *xi;
    uint64_t seed;
    int64_t step, sample_offset;
    float a, k;
    const sp_step_rec* sched;
    const int32_t* cursor;
};

struct ss_epi {
    const float *S, *P;  // Hy x Wy, row-major
    int Hy, Wy;
    const float* q;  // spectral observation rows: (b / y_div) * q_sample + c * Hy * Wy + i * Wy + j
    int64_t q_sample, y_div;
    float gs, rho, scale;
    float* partial;
    const float *x, *xi;  // DiffPIR: rows of n
    uint64_t seed;
    int64_t step, sample_offset;
    sp_prox_coefs pc;
    sp_ddrm_coefs dc;
    const sp_step_rec* sched;
    const int32_t* cursor;
};

struct ld_plain {
    const float* p;
    __device__ __forceinline__ bool aligned() const { return ((uintptr_t)p & 15u) == 0; }
    __device__ __forceinline__ float one(int64_t o) const { return p[o]; }
    __device__ __forceinline__ void four(int64_t o, float (&v)[4]) const { load_v<4>(p + o, v); }
};

// x0 = (x - k eps) / a, every operation rounded on its own
struct ld_x0 {
    const float *x, *e;
    float a, k;
    __device__ __forceinline__ bool aligned() const { return (((uintptr_t)x | (uintptr_t)e) & 15u) == 0; }
    __device__ __forceinline__ float one(int64_t o) const {
#pragma clang fp contract(off)
        return (x[o] - k * e[o]) / a;
    }
    __device__ __forceinline__ void four(int64_t o, float (&v)[4]) const {
        float ev[4];
        load_v<4>(x + o, v);
        load_v<4>(e + o, ev);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma clang fp contract(off)
            v[i] = (v[i] - k * ev[i]) / a;
        }
    }
};

// source 0: x0, 1: eps, 2: xi (read, or Philox at the flat element index el0 + o of the sample)
template <bool XI_IN>
struct ld_ddrm {
    int src;
    ld_x0 x0;
    const float* xi;
    uint64_t seed;
    int64_t step, sample, el0;
    __device__ __forceinline__ bool aligned() const {
        return x0.aligned() && (XI_IN ? ((uintptr_t)xi & 15u) == 0 : (el0 & 3) == 0);
    }
    __device__ __forceinline__ float one(int64_t o) const {
        if (src == 0) return x0.one(o);
        if (src == 1) return x0.e[o];
        if constexpr (XI_IN) return xi[o];
        float z[1];
        philox_normals<1>(seed, step, sample, el0 + o, z);
        return z[0];
    }
    __device__ __forceinline__ void four(int64_t o, float (&v)[4]) const {
        if (src == 0) x0.four(o, v);
        else if (src == 1) load_v<4>(x0.e + o, v);
        else if constexpr (XI_IN) load_v<4>(xi + o, v);
        else philox_normals<4>(seed, step, sample, el0 + o, v);
    }
};

// One LDS tile T[k][mn] of an operand with strides (s_k, s_mn) and extents (K, MN), origin
// (k0, mn0); zeros past the extents.  float4 loads along whichever index is contiguous when the
// plane is 16-byte aligned and the extent and the other stride are multiples of 4.
template <class LD>
__device__ __forceinline__ void ss_fill(float (*T)[kLd], const LD& ld, int64_t lim, int64_t s_mn,
                                        int64_t s_k, int MN, int K, int mn0, int k0) {
    const int t = threadIdx.x;
    const bool al = ld.aligned();
    if (s_mn == 1 && al && MN % 4 == 0 && s_k % 4 == 0) {
        const int g = t & 15, k = t >> 4, mn = mn0 + 4 * g, kk = k0 + k;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (mn < MN && kk < K) {
            SP_DCHECK(kk * s_k + mn + 3 < lim);
            ld.four(kk * s_k + mn, v);
        }
        store_v<4>(&T[k][4 * g], v);
    } else if (s_k == 1 && al && K % 4 == 0 && s_mn % 4 == 0) {
        const int kg = t & 3, m = t >> 2, mn = mn0 + m, kk = k0 + 4 * kg;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (mn < MN && kk < K) {
            SP_DCHECK(mn * s_mn + kk + 3 < lim);
            ld.four(mn * s_mn + kk, v);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) T[4 * kg + e][m] = v[e];
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = s_k == 1 ? (t & 15) : (t >> 6) + 4 * r;
            const int m = s_k == 1 ? (t >> 4) + 16 * r : (t & 63);
            const int mn = mn0 + m, kk = k0 + k;
            float v = 0.f;
            if (mn < MN && kk < K) {
                SP_DCHECK(mn * s_mn + kk * s_k < lim);
                v = ld.one(mn * s_mn + kk * s_k);
            }
            T[k][m] = v;
        }
    }
}

template <int SRC, bool XI_IN, int EPI>
__global__ __launch_bounds__(kBlock) void k_ss_gemm(ss_gemm g, ss_pro pr, ss_epi ep) {
    __shared__ __attribute__((aligned(16))) float smem[kTile * kLd];  // As, Bs; the DiffPIR xi tile
    __shared__ float red4[4];
    float(*As)[kLd] = reinterpret_cast<float(*)[kLd]>(smem);
    float(*Bs)[kLd] = As + kChunk;
    const int64_t plane = blockIdx.x;
    const int tn = (g.N + kTile - 1) / kTile;
    const int ti = static_cast<int>(blockIdx.y) / tn, tj = static_cast<int>(blockIdx.y) - ti * tn;
    const int i0 = ti * kTile, j0 = tj * kTile;
    const int64_t b = plane / g.C;
    const int c = static_cast<int>(plane - b * g.C);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wi = (wid >> 1) * 32, wj = (wid & 1) * 32, half = lane >> 5, l32 = lane & 31;
    SP_DCHECK(i0 < g.M && j0 < g.N && c < g.C);

    if (ep.sched) {  // device-resident schedule (graph replay)
        const sp_dps_coefs& cf = ep.sched[*ep.cursor].c;
        pr.a = cf.a, pr.k = cf.k, ep.gs = cf.grad_scale;
    }

    // the loads of B
    const int64_t boff = b * g.B.sample + c * g.B.plane;
    const float* bp = g.B.p + boff;
    auto make_b = [&]() {
        if constexpr (SRC == SS_SRC_PLAIN) {
            return ld_plain{bp};
        } else if constexpr (SRC == SS_SRC_X0) {
            return ld_x0{bp, pr.eps + boff, pr.a, pr.k};
        } else {
            return ld_ddrm<XI_IN>{static_cast<int>(blockIdx.z),
                                  ld_x0{bp, pr.eps + boff, pr.a, pr.k},
                                  XI_IN ? pr.xi + boff : nullptr,
                                  pr.seed,
                                  pr.step,
                                  pr.sample_offset + b,
                                  (int64_t)c * g.B.plane};
        }
    };
    const auto ldb = make_b();

    constexpr int NS = EPI == SS_DDRM ? 3 : 1;
    f32x16 res = {};
    float fth[EPI == SS_DDRM ? 16 : 1], fep[EPI == SS_DDRM ? 16 : 1], fxi[EPI == SS_DDRM ? 16 : 1];
    if constexpr (EPI == SS_DDRM) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
#pragma clang fp contract(off)
            const int i = i0 + wi + (r >> 2) * 8 + half * 4 + (r & 3), j = j0 + wj + l32;
            const bool obs = i < ep.Hy && j < ep.Wy;
            float s = 0.f, pv = 0.f, qv = 0.f;
            if (obs) {
                const int64_t o = (int64_t)i * ep.Wy + j;
                s = ep.S[o], pv = ep.P[o];
                qv = ep.q[(b / ep.y_div) * ep.q_sample + (int64_t)c * ep.Hy * ep.Wy + o];
            }
            const ddrm_f f = ddrm_class_coefs(ep.dc, s * s, obs && pv != 0.f);
            fth[r] = f.th, fep[r] = f.ep, fxi[r] = f.xi;
            res[r] = f.y * qv;
        }
    }

#pragma unroll
    for (int src = 0; src < NS; ++src) {
        const ld_plain lda{g.A.p + b * g.A.sample + c * g.A.plane + src * g.src_stride};
        f32x16 acc = {};
        for (int k0 = 0; k0 < g.K; k0 += kChunk) {
            ss_fill(As, lda, g.A.lim, g.A.rs, g.A.cs, g.M, g.K, i0, k0);
            ss_fill(Bs, ldb, g.B.lim, g.B.cs, g.B.rs, g.N, g.K, j0, k0);
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < kChunk; kk += 2)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + half][wi + l32], Bs[kk + half][wj + l32],
                                                           acc, 0, 0, 0);
            __syncthreads();
        }
        if constexpr (EPI == SS_DDRM) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
#pragma clang fp contract(off)
                const float f = src == 0 ? fth[r] : src == 1 ? fep[r] : fxi[r];
                res[r] = res[r] + f * acc[r];
            }
        } else {
            res = acc;
        }
    }

    if constexpr (EPI == SS_DIFFPIR) {  // the tile of xi through LDS: one Philox group per 4 elements
        float(*Xi)[kLd] = reinterpret_cast<float(*)[kLd]>(smem);
        const int64_t el0 = (int64_t)c * g.o_plane;  // out: rows of n, planes of H * W, ldo = W
        const int64_t ooff = b * g.o_sample + el0;
        const float* xp = XI_IN ? ep.xi + ooff : nullptr;
        if (g.ldo % 4 == 0 && (el0 & 3) == 0 && (!XI_IN || ((uintptr_t)xp & 15u) == 0)) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int idx = threadIdx.x + r * kBlock, i = idx >> 4, j = (idx & 15) * 4;
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                if (i0 + i < g.M && j0 + j < g.N) {
                    const int64_t o = (int64_t)(i0 + i) * g.ldo + j0 + j;
                    SP_DCHECK(o + 3 < g.o_plane);
                    if constexpr (XI_IN) load_v<4>(xp + o, v);
                    else philox_normals<4>(ep.seed, ep.step, ep.sample_offset + b, el0 + o, v);
                }
                store_v<4>(&Xi[i][j], v);
            }
        } else {
            for (int idx = threadIdx.x; idx < kTile * kTile; idx += kBlock) {
                const int i = idx >> 6, j = idx & 63;
                float v[1] = {0.f};
                if (i0 + i < g.M && j0 + j < g.N) {
                    const int64_t o = (int64_t)(i0 + i) * g.ldo + j0 + j;
                    SP_DCHECK(o < g.o_plane);
                    if constexpr (XI_IN) v[0] = xp[o];
                    else philox_normals<1>(ep.seed, ep.step, ep.sample_offset + b, el0 + o, v);
                }
                Xi[i][j] = v[0];
            }
        }
        __syncthreads();
    }

    const int64_t ooff = b * g.o_sample + c * g.o_plane;
    float* __restrict__ op = g.out + ooff + static_cast<int64_t>(blockIdx.z) * g.src_stride;
    const int64_t qbase = (b / ep.y_div) * ep.q_sample + (int64_t)c * ep.Hy * ep.Wy;
    const float inv_k = EPI == SS_DIFFPIR ? 1.f / ep.pc.k : 1.f;
    float rsq = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma clang fp contract(off)
        const int il = wi + (r >> 2) * 8 + half * 4 + (r & 3), jl = wj + l32;
        const int i = i0 + il, j = j0 + jl;
        if (i < g.M && j < g.N) {
            const float d = res[r];
            const int64_t to = (int64_t)i * ep.Wy + j;  // S, P, q: where i < Hy and j < Wy
            float o = d;
            if constexpr (EPI == SS_MUL) {
                o = d * ep.S[to];
            } else if constexpr (EPI == SS_SCALE) {
                o = ep.scale * d;
            } else if constexpr (EPI == SS_DPS) {
                const float s = ep.S[to];
                const float rr = ep.q[qbase + to] - s * d;
                rsq += rr * rr;
                o = ep.gs * (s * rr);
            } else if constexpr (EPI == SS_PGDM) {
                o = ep.gs * (ep.q[qbase + to] - (ep.P[to] != 0.f ? d : 0.f));
            } else if constexpr (EPI == SS_PROX) {
                if (i < ep.Hy && j < ep.Wy) {
                    const float s = ep.S[to];
                    o = (ep.q[qbase + to] + ep.rho * d) / (s * s + ep.rho);
                }
            } else if constexpr (EPI == SS_DIFFPIR) {
                const float(*Xi)[kLd] = reinterpret_cast<const float(*)[kLd]>(smem);
                const float xv = ep.x[ooff + (int64_t)i * g.ldo + j];
                o = diffpir_update(ep.pc, inv_k, xv, d, Xi[il][jl]);
            }
            SP_DCHECK((int64_t)i * g.ldo + j < g.o_plane);
            op[(int64_t)i * g.ldo + j] = o;
        }
    }
    if constexpr (EPI == SS_DPS) {
        const float tot = block_sum(rsq, red4);
        const int tiles = static_cast<int>(gridDim.y);
        if (threadIdx.x == 0)
            ep.partial[b * ((int64_t)g.C * tiles) + (int64_t)c * tiles + blockIdx.y] = tot;
    }
}

struct ss_geom {
    int C, H, W, Hy, Wy;
    int64_t HW, m;
    const float *VH, *VW, *UH, *UW, *S, *P;
};

ss_geom ss_geom_of(const sp_op* op) {
    ss_geom g;
    g.C = op->channels, g.H = op->height, g.W = op->width, g.Hy = op->radius, g.Wy = op->factor;
    g.HW = (int64_t)g.H * g.W, g.m = op->m;
    g.VH = op->taps;
    g.VW = g.VH + (int64_t)g.H * g.H;
    g.UH = g.VW + (int64_t)g.W * g.W;
    g.UW = g.UH + (int64_t)g.Hy * g.Hy;
    g.S = g.UW + (int64_t)g.Wy * g.Wy;
    g.P = g.S + (int64_t)g.Hy * g.Wy;
    return g;
}

// op(tab) on the left: D (M x N) = tab[:, :M]^T X (tr) or tab[:, :K] X, tab row-major with ld floats a row
ss_gemm ss_left(const float* tab, int ld, bool tr, int M, int K, const float* X, int64_t xplane, int ldx,
                int N, float* out, int64_t oplane, int ldo, int C) {
    const ss_mat A = {tab, 0, 0, tr ? 1 : ld, tr ? ld : 1,
                      tr ? (int64_t)(K - 1) * ld + M : (int64_t)(M - 1) * ld + K};
    const ss_mat B = {X, C * xplane, xplane, ldx, 1, (int64_t)(K - 1) * ldx + N};
    return {A, B, M, N, K, out, C * oplane, oplane, ldo, C, 0};
}

// on the right: D = X tab[:, :N] or X tab[:, :K]^T (tr)
ss_gemm ss_right(const float* X, int64_t xplane, int ldx, int M, int K, const float* tab, int ld, bool tr,
                 int N, float* out, int64_t oplane, int ldo, int C) {
    const ss_mat A = {X, C * xplane, xplane, ldx, 1, (int64_t)(M - 1) * ldx + K};
    const ss_mat B = {tab, 0, 0, tr ? 1 : ld, tr ? ld : 1,
                      tr ? (int64_t)(N - 1) * ld + K : (int64_t)(K - 1) * ld + N};
    return {A, B, M, N, K, out, C * oplane, oplane, ldo, C, 0};
}

template <int SRC, bool XI_IN, int EPI>
void ss_run(const ss_gemm& g, const ss_pro& pr, const ss_epi& ep, int64_t planes, int nsrc, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>(planes),
                    static_cast<unsigned>(cdiv(g.M, kTile) * cdiv(g.N, kTile)), static_cast<unsigned>(nsrc));
    launch(0, k_ss_gemm<SRC, XI_IN, EPI>, grid, dim3(kBlock), s, g, pr, ep);
}

void ss_plain(const ss_gemm& g, int64_t planes, hipStream_t s) {
    ss_epi ep = {};
    ep.y_div = 1;
    ss_run<SS_SRC_PLAIN, true, SS_STORE>(g, ss_pro{}, ep, planes, 1, s);
}

ss_epi ss_epi_of(const ss_geom& g, const float* q, int64_t q_sample, int64_t y_div) {
    ss_epi ep = {};
    ep.S = g.S, ep.P = g.P, ep.Hy = g.Hy, ep.Wy = g.Wy;
    ep.q = q, ep.q_sample = q_sample, ep.y_div = y_div;
    return ep;
}

// the observed grid from x-space: L V_H[:, :Hy]^T in -> W0 (x0 in the loads with pr), then
// R W0 V_W[:, :Wy] with the epilogue EPI -> dst (planes of H * W, rows of Wy)
template <int EPI>
void ss_to_obs(const ss_geom& g, const float* in, const ss_pro* pr, const ss_epi& ep, float* W0, float* dst,
               int64_t batch, hipStream_t s) {
    const int64_t planes = batch * g.C;
    const ss_gemm l = ss_left(g.VH, g.H, true, g.Hy, g.H, in, g.HW, g.W, g.W, W0, g.HW, g.W, g.C);
    ss_epi e0 = {};
    e0.y_div = 1;
    if (pr) {
        e0.sched = ep.sched, e0.cursor = ep.cursor;
        ss_run<SS_SRC_X0, true, SS_STORE>(l, *pr, e0, planes, 1, s);
    } else {
        ss_run<SS_SRC_PLAIN, true, SS_STORE>(l, ss_pro{}, e0, planes, 1, s);
    }
    ss_run<SS_SRC_PLAIN, true, EPI>(
        ss_right(W0, g.HW, g.W, g.Hy, g.W, g.VW, g.W, false, g.Wy, dst, g.HW, g.Wy, g.C), ss_pro{}, ep,
        planes, 1, s);
}

// x-space from the observed grid: L V_H[:, :Hy] src -> W0, R W0 V_W[:, :Wy]^T -> out
void ss_from_obs(const ss_geom& g, const float* src, float* W0, float* out, int64_t batch, hipStream_t s) {
    const int64_t planes = batch * g.C;
    ss_plain(ss_left(g.VH, g.H, false, g.H, g.Hy, src, g.HW, g.Wy, g.Wy, W0, g.HW, g.Wy, g.C), planes, s);
    ss_plain(ss_right(W0, g.HW, g.Wy, g.H, g.Wy, g.VW, g.W, true, g.W, out, g.HW, g.W, g.C), planes, s);
}

// T_y of `rows` observation rows (planes of Hy * Wy) -> dst (the same planes, a row every `stride`
// floats), through scratch (likewise), times the table `mul` (null: none)
void ss_ty(const ss_geom& g, const float* y, int64_t rows, const float* mul, float* scratch, float* dst,
           int64_t stride, hipStream_t s) {
    const int64_t planes = rows * g.C, yp = (int64_t)g.Hy * g.Wy;
    ss_gemm l = ss_left(g.UH, g.Hy, true, g.Hy, g.Hy, y, yp, g.Wy, g.Wy, scratch, yp, g.Wy, g.C);
    l.o_sample = stride;
    ss_plain(l, planes, s);
    ss_gemm r = ss_right(scratch, yp, g.Wy, g.Hy, g.Wy, g.UW, g.Wy, false, g.Wy, dst, yp, g.Wy, g.C);
    r.A.sample = r.o_sample = stride;
    if (mul) {
        ss_epi ep = ss_epi_of(g, nullptr, 0, 1);
        ep.S = mul;
        ss_run<SS_SRC_PLAIN, true, SS_MUL>(r, ss_pro{}, ep, planes, 1, s);
    } else {
        ss_plain(r, planes, s);
    }
}

}  // namespace

bool svd_sep_valid(const sp_op* op) {
    return op->taps && !op->keep_bits && !op->word_rank && op->channels >= 1 && op->height >= 2 &&
           op->height <= 512 && op->width >= 2 && op->width <= 512 && op->radius >= 1 &&
           op->radius <= op->height && op->factor >= 1 && op->factor <= op->width &&
           op->n == (int64_t)op->channels * op->height * op->width &&
           op->m == (int64_t)op->channels * op->radius * op->factor;
}

int64_t svd_sep_partials(const sp_op* op) {
    return (int64_t)op->channels * cdiv(op->radius, kTile) * cdiv(op->factor, kTile);
}

int64_t svd_sep_op_workspace(const sp_op* op, int64_t batch) { return 2 * batch * op->n; }
int64_t svd_sep_dps_workspace(const sp_op* op, int64_t batch) { return 3 * batch * op->n; }
int64_t svd_sep_ddrm_workspace(const sp_op* op, int64_t batch) { return 4 * batch * op->n; }

// A (transpose of A^+ with P) and A^T (A^+ with P)
static int ss_forward(const sp_op* op, const float* x, float* y, int64_t batch, const float* mul, float* work,
                      hipStream_t s) {
    const ss_geom g = ss_geom_of(op);
    float *W0 = work, *W1 = work + batch * op->n;
    ss_epi ep = ss_epi_of(g, nullptr, 0, 1);
    ep.S = mul;
    ss_to_obs<SS_MUL>(g, x, nullptr, ep, W0, W1, batch, s);
    const int64_t planes = batch * g.C;
    ss_plain(ss_left(g.UH, g.Hy, false, g.Hy, g.Hy, W1, g.HW, g.Wy, g.Wy, W0, g.HW, g.Wy, g.C), planes, s);
    ss_plain(ss_right(W0, g.HW, g.Wy, g.Hy, g.Wy, g.UW, g.Wy, true, g.Wy, y, (int64_t)g.Hy * g.Wy, g.Wy, g.C),
             planes, s);
    return check_launch("svd_separable forward");
}

static int ss_backward(const sp_op* op, const float* gy, float* dx, int64_t batch, const float* mul,
                       float* work, hipStream_t s) {
    const ss_geom g = ss_geom_of(op);
    float *W0 = work, *W1 = work + batch * op->n;
    const int64_t planes = batch * g.C, yp = (int64_t)g.Hy * g.Wy;
    ss_plain(ss_left(g.UH, g.Hy, true, g.Hy, g.Hy, gy, yp, g.Wy, g.Wy, W0, g.HW, g.Wy, g.C), planes, s);
    ss_epi ep = ss_epi_of(g, nullptr, 0, 1);
    ep.S = mul;
    ss_run<SS_SRC_PLAIN, true, SS_MUL>(
        ss_right(W0, g.HW, g.Wy, g.Hy, g.Wy, g.UW, g.Wy, false, g.Wy, W1, g.HW, g.Wy, g.C), ss_pro{}, ep,
        planes, 1, s);
    ss_from_obs(g, W1, W0, dx, batch, s);
    return check_launch("svd_separable backward");
}

int svd_sep_apply(const sp_op* op, const float* x, float* y, int64_t batch, float* work, hipStream_t s) {
    return ss_forward(op, x, y, batch, ss_geom_of(op).S, work, s);
}

int svd_sep_vjp(const sp_op* op, const float*, const float* gy, float* dx, int64_t batch, float* work,
                hipStream_t s) {
    return ss_backward(op, gy, dx, batch, ss_geom_of(op).S, work, s);
}

int svd_sep_pinv(const sp_op* op, const float* y, float* x, int64_t batch, int transpose, float* work,
                 hipStream_t s) {
    const float* P = ss_geom_of(op).P;
    return transpose ? ss_forward(op, y, x, batch, P, work, s) : ss_backward(op, y, x, batch, P, work, s);
}

int svd_sep_pgdm_prepare(const sp_op* op, const float* y, int64_t rows, float* q, hipStream_t s) {
    const ss_geom g = ss_geom_of(op);
    ss_ty(g, y, rows, g.P, q + op->m, q, 2 * op->n, s);
    return check_launch("sp_pgdm_prepare");
}

int svd_sep_prox_prepare(const sp_op* op, const float* y, int64_t rows, float* q, hipStream_t s) {
    const ss_geom g = ss_geom_of(op);
    ss_ty(g, y, rows, g.S, q + op->m, q, 2 * op->n, s);
    return check_launch("sp_prox_prepare");
}

int svd_sep_dps_residual(const sp_op* op, const dps_residual_args& r, hipStream_t s) {
    const ss_geom g = ss_geom_of(op);
    float *W0 = r.work, *W1 = W0 + r.batch * op->n, *W2 = W1 + r.batch * op->n;
    ss_ty(g, r.y, cdiv(r.batch, r.y_div), nullptr, W0, W2, op->m, s);
    const ss_pro pr = {r.eps, nullptr, 0, 0, 0, r.a, r.k, r.sched, r.cursor};
    ss_epi ep = ss_epi_of(g, W2, op->m, r.y_div);
    ep.gs = r.gs, ep.partial = r.partial, ep.sched = r.sched, ep.cursor = r.cursor;
    ss_to_obs<SS_DPS>(g, r.x, &pr, ep, W0, W1, r.batch, s);
    ss_from_obs(g, W1, W0, r.v, r.batch, s);
    return check_launch("sp_dps_residual (svd_separable)");
}

int svd_sep_pgdm_residual(const sp_op* op, const float* x, const float* eps, const float* q, int64_t batch,
                          int64_t y_div, const sp_dps_coefs& c, float* v, float* work, hipStream_t s) {
    const ss_geom g = ss_geom_of(op);
    float *W0 = work, *W1 = W0 + batch * op->n;
    const ss_pro pr = {eps, nullptr, 0, 0, 0, c.a, c.k, nullptr, nullptr};
    ss_epi ep = ss_epi_of(g, q, 2 * op->n, y_div);
    ep.gs = c.grad_scale;
    ss_to_obs<SS_PGDM>(g, x, &pr, ep, W0, W1, batch, s);
    ss_from_obs(g, W1, W0, v, batch, s);
    return check_launch("sp_pgdm_residual_ws (svd_separable)");
}

// both forms: p.eps selects the whole DiffPIR step
int svd_sep_prox(const sp_op* op, const prox_args& p, hipStream_t s) {
    const ss_geom g = ss_geom_of(op);
    float *W0 = p.work, *W1 = W0 + p.batch * op->n;
    const int64_t planes = p.batch * g.C;
    const ss_gemm l1 = ss_left(g.VH, g.H, true, g.H, g.H, p.x, g.HW, g.W, g.W, W0, g.HW, g.W, g.C);
    ss_epi e0 = {};
    e0.y_div = 1;
    if (p.eps)
        ss_run<SS_SRC_X0, true, SS_STORE>(l1, ss_pro{p.eps, nullptr, 0, 0, 0, p.c.a, p.c.k, nullptr, nullptr}, e0,
                                          planes, 1, s);
    else
        ss_run<SS_SRC_PLAIN, true, SS_STORE>(l1, ss_pro{}, e0, planes, 1, s);
    ss_epi ep = ss_epi_of(g, p.q, 2 * op->n, p.y_div);
    ep.rho = p.c.rho;
    ss_run<SS_SRC_PLAIN, true, SS_PROX>(
        ss_right(W0, g.HW, g.W, g.H, g.W, g.VW, g.W, false, g.W, W1, g.HW, g.W, g.C), ss_pro{}, ep, planes, 1, s);
    ss_plain(ss_left(g.VH, g.H, false, g.H, g.H, W1, g.HW, g.W, g.W, W0, g.HW, g.W, g.C), planes, s);
    const ss_gemm r2 = ss_right(W0, g.HW, g.W, g.H, g.W, g.VW, g.W, true, g.W, p.out, g.HW, g.W, g.C);
    if (p.eps) {
        ss_epi ed = {};
        ed.y_div = 1, ed.x = p.x, ed.xi = p.xi, ed.seed = p.seed, ed.step = p.step;
        ed.sample_offset = p.sample_offset, ed.pc = p.c;
        select_bool(p.xi, [&](auto xin) { ss_run<SS_SRC_PLAIN, xin(), SS_DIFFPIR>(r2, ss_pro{}, ed, planes, 1, s); });
    } else {
        ss_plain(r2, planes, s);
    }
    return check_launch(p.eps ? "sp_diffpir_step_ws (svd_separable)" : "sp_op_prox_ws (svd_separable)");
}

int svd_sep_ddrm(const sp_op* op, const ddrm_args& p, hipStream_t s) {
    const ss_geom g = ss_geom_of(op);
    const int64_t stride = p.batch * op->n, planes = p.batch * g.C;
    float *W0 = p.work, *W3 = W0 + 3 * stride;
    ss_gemm l1 = ss_left(g.VH, g.H, true, g.H, g.H, p.x, g.HW, g.W, g.W, W0, g.HW, g.W, g.C);
    l1.src_stride = stride;
    const ss_pro pr = {p.eps, p.xi, p.seed, p.step, p.sample_offset, p.c.a, p.c.k, nullptr, nullptr};
    ss_epi e0 = {};
    e0.y_div = 1;
    select_bool(p.xi, [&](auto xin) { ss_run<SS_SRC_DDRM, xin(), SS_STORE>(l1, pr, e0, planes, 3, s); });
    ss_gemm r1 = ss_right(W0, g.HW, g.W, g.H, g.W, g.VW, g.W, false, g.W, W3, g.HW, g.W, g.C);
    r1.src_stride = stride;
    ss_epi ep = ss_epi_of(g, p.q, 2 * op->n, p.y_div);
    ep.dc = p.c;
    ss_run<SS_SRC_PLAIN, true, SS_DDRM>(r1, ss_pro{}, ep, planes, 1, s);
    r1.src_stride = 0;
    ss_plain(ss_left(g.VH, g.H, false, g.H, g.H, W3, g.HW, g.W, g.W, W0, g.HW, g.W, g.C), planes, s);
    ss_epi es = {};
    es.y_div = 1, es.scale = p.c.a_prev;
    ss_run<SS_SRC_PLAIN, true, SS_SCALE>(
        ss_right(W0, g.HW, g.W, g.H, g.W, g.VW, g.W, true, g.W, p.out, g.HW, g.W, g.C), ss_pro{}, es, planes, 1, s);
    return check_launch("sp_ddrm_step_ws (svd_separable)");
}

}  // namespace sp
