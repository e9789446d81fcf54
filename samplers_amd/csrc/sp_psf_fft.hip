// FFT-domain point-spread-function blur (SP_OP_PSF_FFT): the correlation of SP_OP_PSF,
//   y[c,i,j] = sum_{u,v} h[u,v] xe[c, i+u, j+v],  0 <= u, v < K = 2R + 1,
// with xe the image extended by R on each side by reflection, wrap-around or zeros
// (op.factor = 0, 1, 2), evaluated through circular transforms of Nh x Nw points, Nh (Nw) the
// smallest 2^k or 3 * 2^k in [8, 1024] that holds H + 2R (W + 2R).  Semantics in
// operators/psf_fft.py, pinned in fp64 by tests/psf_fft_ops.py.  With xe at [0, H+2R) x [0, W+2R)
// of a zero Nh x Nw array and Hs = FFT2 of h at [0, K) x [0, K) (op.taps, the caller's):
//   A x   = IFFT2(FFT2(xe) * conj(Hs)) [0, H) x [0, W)          (no index wraps: i + u < Nh)
//   A^T g = fold(IFFT2(FFT2(g at [0, H) x [0, W)) * Hs) [0, H+2R) x [0, W+2R))
// where fold is the transpose of the extension: every extended position is added onto the pixel
// it was copied from (zeros: the margin is dropped).
//
// Three launches through the caller's workspace, as SP_OP_PHASE (sp_phase.hip), with the FFT core
// of sp_fft.h:
//   1. rows     a workgroup stages TR rows of one plane (x0 = (x - k eps) / a in DPS form),
//               extended W -> W + 2R by the mode's index function (A) or as they are (A^T),
//               zero-extended to Nw; Nw-point FFT per row; columns kw <= Nw / 2 stored TRANSPOSED
//               (the rows are real: the other half is the conjugate mirror).
//   2. columns  a workgroup loads TC columns of H values, extends H -> H + 2R by the same index
//               function in LDS (A; the row transform is linear, so extending the rows after it is
//               exact), zero-extends to Nh; forward FFT; times conj(Hs) / (Nh Nw) (A) or
//               Hs / (Nh Nw) (A^T); inverse FFT; rows 0 .. H-1 (A) or positions 0 .. H+2R-1 folded
//               onto the H rows (A^T) stored back over the columns it loaded.
//   3. rows^-1  TR rows of the intermediate -> LDS, kw > Nw / 2 rebuilt by conjugate symmetry,
//               inverse FFT, real part; columns 0 .. W-1 (A) or 0 .. W+2R-1 folded onto W (A^T).
// DPS pass 1 is five launches: rows, columns (A), rows^-1 fused with rows (the block holds the
// rows of A x0 in LDS, forms g = grad_scale (y - A x0) and its r^2 partial, zero-extends g and
// transforms it forward again in place), columns (A^T), rows^-1 (A^T) -> v.
//
// Intermediate: complex fp32 (re, im), [sample][plane][Nw / 2 + 1][H];
// 2 * batch * C * (Nw / 2 + 1) * H floats.  Spectrum (op.taps): (re, im) pairs [Nw / 2 + 1][Nh],
// so a column tile reads one contiguous run.
//
// A fold adds its at most three terms in a fixed order: interior, low-border image, high-border
// image (1 <= R <= min(H, W) - 1 bounds the pre-images per axis by three).  Every sample is
// computed alone, lines are assigned by plane and tile only, the r^2 partial of a
// (plane, row tile) is block_sum's fixed order: the bits do not depend on the batch, y_div or the
// shard.  Plain stores, no atomics.
//
// SP_OP_PSF_PERIODIC runs the same kernels on exact-size transforms, Nh = H and Nw = W, where the
// wrap-around blur is diagonal: nothing extended or folded, and a pseudo-inverse that is one more
// multiplier.  The host section at the end of the file launches both kinds through one pipeline.
// SP_OP_SR_PERIODIC (the k_srp_* kernels below and the last host section) puts the lattice
// [::s, ::s] between the periodic kind's transforms: blur-and-decimate super-resolution.

#include <algorithm>

#define SP_TU 18  // debug-build site numbering (sp_common.h SP_DCHECK)
#include "sp_ops.h"
#include "sp_fft.h"

namespace sp {

enum { PF_REFLECT = 0, PF_CIRCULAR = 1, PF_ZEROS = 2 };
enum { PF_OUT_A = 0, PF_OUT_AT = 1, PF_OUT_RESIDUAL = 2, PF_OUT_PROX = 3, PF_OUT_PROX_ADD = 4, PF_OUT_SCALE = 5 };
enum { PF_COL_MAP = 0, PF_COL_PREPARE = 1, PF_COL_PGDM = 2, PF_COL_PROX = 3 };

// what the PF_OUT_PROX epilogue of k_pf_rows_inv needs besides z (the other forms pass an empty
// one): step != 0 forms eps_hat from x and writes the DiffPIR sample, else z itself.
// PF_OUT_PROX_ADD (SP_OP_SR_PERIODIC): the transform holds z - x0, and x0 (x itself, or
// (x - k eps) / a in the step form) is added in space first
struct pf_prox_tail {
    const float *x, *xi, *eps;
    uint64_t seed;
    int64_t step, sample_offset;
    sp_prox_coefs c;
    int step_form;
};

// smallest 2^k or 3 * 2^k in [8, 1024] that is >= n; 0 if there is none
static int pf_size(int n) {
    for (int N = n < 8 ? 8 : n; N <= 1024; ++N)
        if (phase_size_ok(N)) return N;
    return 0;
}

struct pf_geom {  // filled on the host from a valid descriptor (pf_geometry)
    int C, H, W, R, mode, Nh, Nw, HW;  // HW = Nw / 2 + 1 stored columns
    const float2* spec;                // [HW][Nh]
    int s;                             // SP_OP_SR_PERIODIC: the lattice stride (1 for the others)
    const float* lam;                  // SP_OP_SR_PERIODIC: Lambda_t [HW][Nh]
};

// source pixel of extended position p in [0, n + 2R) along an axis of n pixels; -1: a zero
__device__ __forceinline__ int pf_src(int p, int R, int n, int mode) {
    const int i = p - R;
    if (i >= 0 && i < n) return i;
    if (mode == PF_ZEROS) return -1;
    if (mode == PF_REFLECT) return i < 0 ? -i : 2 * (n - 1) - i;
    return i < 0 ? i + n : i - n;
}

// the extended positions besides R + i that pf_src maps to pixel i: one in the low border
// [0, R), one in the high border [n + R, n + 2R), -1 where there is none
__device__ __forceinline__ void pf_images(int i, int R, int n, int mode, int& lo, int& hi) {
    lo = hi = -1;
    if (mode == PF_REFLECT) {
        if (i >= 1 && i <= R) lo = R - i;
        if (i >= n - 1 - R && i <= n - 2) hi = R + 2 * (n - 1) - i;
    } else if (mode == PF_CIRCULAR) {
        if (i >= n - R) lo = R + i - n;
        if (i < R) hi = R + i + n;
    }
}

// launch 1.  X0: x0 = (in - k eps) / a while staging.  EXT: extend by the mode (A), else the row
// as it is at [0, W) (A^T).
template <bool X0, bool EXT>
__global__ __launch_bounds__(kBlock) void k_pf_rows(pf_geom g, const float* __restrict__ in,
                                                    const float* __restrict__ eps, float a, float k,
                                                    float2* __restrict__ ws, int T,
                                                    const sp_step_rec* __restrict__ sched,
                                                    const int32_t* __restrict__ cursor) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if (X0 && sched) {  // device-resident schedule (graph replay)
        const sp_dps_coefs& cf = sched[*cursor].c;
        a = cf.a, k = cf.k;
    }
    const int N = g.Nw, NP = phase_np(N);
    float2* tw = reinterpret_cast<float2*>(smem);
    float2* A = tw + N;
    float2* B = A + T * NP;
    const int tiles = (g.H + T - 1) / T;
    const int c = static_cast<int>(blockIdx.x) / tiles;
    const int h0 = (static_cast<int>(blockIdx.x) - c * tiles) * T;
    const int64_t plane = (int64_t)blockIdx.y * g.C + c;
    SP_DCHECK(c < g.C && h0 < g.H);
    const float* __restrict__ ip = in + plane * g.H * g.W;
    const float* __restrict__ ep = X0 ? eps + plane * g.H * g.W : nullptr;
    const int ext = EXT ? g.W + 2 * g.R : g.W;

    phase_twiddles(tw, N);
    for (int t = 0; t < T; ++t) {
        const int h = h0 + t;
        for (int q = threadIdx.x; q < N; q += kBlock) {
            float val = 0.f;
            const int j = q < ext ? (EXT ? pf_src(q, g.R, g.W, g.mode) : q) : -1;
            if (h < g.H && j >= 0) {
                SP_DCHECK(j < g.W && h * g.W + j < g.H * g.W);
                val = ip[h * g.W + j];
                if constexpr (X0) val = (val - k * ep[h * g.W + j]) / a;
            }
            A[t * NP + phase_slot(q)] = make_float2(val, 0.f);
        }
    }
    __syncthreads();
    const float2* res = phase_fft(A, B, tw, N, NP, T, false);
    // transposed store of the half spectrum: ws[plane][kw][h], the tile's rows adjacent
    float2* __restrict__ wp = ws + plane * (int64_t)g.HW * g.H;
    const int total = T * g.HW;
    for (int idx = threadIdx.x; idx < total; idx += kBlock) {
        const int kw = idx / T, t = idx - kw * T, h = h0 + t;
        if (h < g.H) {
            SP_DCHECK(kw < g.HW && kw * g.H + h < g.HW * g.H);
            wp[kw * g.H + h] = res[t * NP + phase_slot(kw)];
        }
    }
}

// launch 2.  ADJ false: A (extend, conj(Hs), keep rows 0 .. H-1); true: A^T (Hs, fold).
// EXT false: the periodic kind (SP_OP_PSF_PERIODIC, below) - Nh == H, nothing to extend or fold,
// g.spec is the map's own multiplier (ADJ: its conjugate).  FORM (EXT false only):
//   PF_COL_PREPARE  forward transform, times spec / (Nh Nw), stored as the spectrum it is
//                   (sp_pgdm_prepare: Q = P * FFT2(y));
//   PF_COL_PGDM     z <- gs (Q[b / y_div] - (spec != 0 ? z / (Nh Nw) : 0)) between the transforms
//                   (sp_pgdm_residual_ws: spec = P, so spec != 0 is the kept set);
//   PF_COL_PROX     z <- (Q[b / y_div] + rho z / (Nh Nw)) / (|spec|^2 + rho) between the transforms
//                   (the proximal map: spec = M, Q = conj(M) FFT2(y) / (Nh Nw), gs carries rho).
// PF_COL_PREPARE with ADJ is the same launch with the multiplier conjugated (sp_prox_prepare).
template <bool ADJ, bool EXT = true, int FORM = PF_COL_MAP>
__global__ __launch_bounds__(kBlock) void k_pf_cols(pf_geom g, float2* __restrict__ ws, int T,
                                                    const float2* __restrict__ qs, int64_t y_div,
                                                    float gs) {
    static_assert(EXT ? FORM == PF_COL_MAP : (FORM == PF_COL_MAP || FORM == PF_COL_PREPARE || !ADJ),
                  "forms of the periodic kind");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int N = g.Nh, NP = phase_np(N);
    float2* tw = reinterpret_cast<float2*>(smem);
    float2* A = tw + N;
    float2* B = A + T * NP;
    const int tiles = (g.HW + T - 1) / T;
    const int c = static_cast<int>(blockIdx.x) / tiles;
    const int kw0 = (static_cast<int>(blockIdx.x) - c * tiles) * T;
    const int64_t plane = (int64_t)blockIdx.y * g.C + c;
    SP_DCHECK(c < g.C && kw0 < g.HW && (EXT || N == g.H));
    float2* __restrict__ wp = ws + (plane * g.HW + kw0) * (int64_t)g.H;  // the tile's columns
    const int lines = min(T, g.HW - kw0);
    const int ext = ADJ || !EXT ? g.H : g.H + 2 * g.R;

    phase_twiddles(tw, N);
    for (int t = 0; t < T; ++t)
        for (int q = threadIdx.x; q < N; q += kBlock) {
            float2 val = make_float2(0.f, 0.f);
            const int h = q < ext ? (ADJ || !EXT ? q : pf_src(q, g.R, g.H, g.mode)) : -1;
            if (t < lines && h >= 0) {
                SP_DCHECK(h < g.H);
                val = wp[t * g.H + h];
            }
            A[t * NP + phase_slot(q)] = val;
        }
    __syncthreads();
    float2* z = phase_fft(A, B, tw, N, NP, T, false);

    // times the PSF's spectrum (its conjugate for the correlation) and both inverse transforms'
    // 1 / (Nh Nw); the spectrum's columns are contiguous
    const float s = 1.f / ((float)g.Nh * (float)g.Nw);
    const float2* __restrict__ hsp = g.spec + (int64_t)kw0 * N;
    const int total = lines * N;
    if constexpr (FORM == PF_COL_PGDM) {
        const int64_t qplane = ((int64_t)blockIdx.y / y_div) * g.C + c;
        const float2* __restrict__ qp = qs + (qplane * g.HW + kw0) * (int64_t)N;
        for (int idx = threadIdx.x; idx < total; idx += kBlock) {
            const int t = idx / N, kh = idx - t * N;
            SP_DCHECK(t < lines && kw0 + t < g.HW && kh < g.H);
            const float2 p = hsp[idx], qv = qp[idx];
            float2* zp = z + t * NP + phase_slot(kh);
            const bool kept = p.x != 0.f || p.y != 0.f;
            const float2 pz = kept ? make_float2(s * zp->x, s * zp->y) : make_float2(0.f, 0.f);
            *zp = make_float2(gs * (qv.x - pz.x), gs * (qv.y - pz.y));
        }
    } else if constexpr (FORM == PF_COL_PROX) {
        const int64_t qplane = ((int64_t)blockIdx.y / y_div) * g.C + c;
        const float2* __restrict__ qp = qs + (qplane * g.HW + kw0) * (int64_t)N;
        const float rs = gs * s;  // rho / (Nh Nw)
        for (int idx = threadIdx.x; idx < total; idx += kBlock) {
            const int t = idx / N, kh = idx - t * N;
            SP_DCHECK(t < lines && kw0 + t < g.HW && kh < g.H);
            const float2 m = hsp[idx], qv = qp[idx];
            float2* zp = z + t * NP + phase_slot(kh);
            const float inv = 1.f / ((m.x * m.x + m.y * m.y) + gs);
            *zp = make_float2((qv.x + rs * zp->x) * inv, (qv.y + rs * zp->y) * inv);
        }
    } else {
        constexpr bool CONJ = EXT ? !ADJ : ADJ;
        for (int idx = threadIdx.x; idx < total; idx += kBlock) {
            const int t = idx / N, kh = idx - t * N;
            SP_DCHECK(t < lines && kw0 + t < g.HW);
            float2 hs = hsp[idx];
            hs.x *= s;
            hs.y *= CONJ ? -s : s;
            float2* zp = z + t * NP + phase_slot(kh);
            if constexpr (FORM == PF_COL_PREPARE) {
                SP_DCHECK(idx < lines * g.H);
                wp[idx] = cmul(*zp, hs);  // N == H: the spectrum fills the columns it came from
            } else {
                *zp = cmul(*zp, hs);
            }
        }
    }
    if constexpr (FORM == PF_COL_PREPARE) return;
    __syncthreads();
    const float2* u = phase_fft(z, z == A ? B : A, tw, N, NP, T, true);
    const int keep = lines * g.H;
    for (int idx = threadIdx.x; idx < keep; idx += kBlock) {
        const int t = idx / g.H, h = idx - t * g.H;
        const float2* ul = u + t * NP;
        float2 val;
        if constexpr (ADJ && EXT) {
            int lo, hi;
            pf_images(h, g.R, g.H, g.mode, lo, hi);
            SP_DCHECK(g.R + h < N && lo < g.R && (hi < 0 || (hi >= g.H + g.R && hi < g.H + 2 * g.R)));
            val = ul[phase_slot(g.R + h)];
            if (lo >= 0) val = cadd(val, ul[phase_slot(lo)]);
            if (hi >= 0) val = cadd(val, ul[phase_slot(hi)]);
        } else {
            val = ul[phase_slot(h)];
        }
        wp[idx] = val;
    }
}

// launch 3.  OUT: PF_OUT_A columns 0 .. W-1 -> out; PF_OUT_AT columns 0 .. W+2R-1 folded onto W
// -> out; PF_OUT_RESIDUAL the fused launch of DPS pass 1: g = gs (y - A x0) and the r^2 partial
// of the tile, then the forward row transform of g back into the intermediate; PF_OUT_SCALE
// (the DDRM step's launch 3) gs times the real part -> out, on PF_OUT_PROX's float4 path.
template <int OUT>
__global__ __launch_bounds__(kBlock) void k_pf_rows_inv(pf_geom g, float2* __restrict__ ws,
                                                        float* __restrict__ out,
                                                        const float* __restrict__ y, int64_t y_div,
                                                        float gs, float* __restrict__ partial, int P,
                                                        int T, const sp_step_rec* __restrict__ sched,
                                                        const int32_t* __restrict__ cursor,
                                                        pf_prox_tail px) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float red[4];
    if (OUT == PF_OUT_RESIDUAL && sched) gs = sched[*cursor].c.grad_scale;
    const int N = g.Nw, NP = phase_np(N);
    float2* tw = reinterpret_cast<float2*>(smem);
    float2* A = tw + N;
    float2* B = A + T * NP;
    const int tiles = (g.H + T - 1) / T;
    const int c = static_cast<int>(blockIdx.x) / tiles;
    const int h0 = (static_cast<int>(blockIdx.x) - c * tiles) * T;
    const int64_t b = blockIdx.y;
    const int64_t plane = b * g.C + c;
    SP_DCHECK(c < g.C && h0 < g.H && (OUT != PF_OUT_RESIDUAL || static_cast<int>(blockIdx.x) < P));
    float2* __restrict__ wp = ws + plane * (int64_t)g.HW * g.H;

    phase_twiddles(tw, N);
    const int total = T * g.HW;
    for (int idx = threadIdx.x; idx < total; idx += kBlock) {
        const int kw = idx / T, t = idx - kw * T, h = h0 + t;
        float2 val = make_float2(0.f, 0.f);
        if (h < g.H) {
            SP_DCHECK(kw < g.HW && kw * g.H + h < g.HW * g.H);
            val = wp[kw * g.H + h];
        }
        A[t * NP + phase_slot(kw)] = val;
        if (kw > 0 && 2 * kw < N) {  // the spectrum of a real row: X[N - kw] = conj(X[kw])
            SP_DCHECK(N - kw >= g.HW && N - kw < N);
            A[t * NP + phase_slot(N - kw)] = make_float2(val.x, -val.y);
        }
    }
    __syncthreads();
    float2* res = phase_fft(A, B, tw, N, NP, T, true);

    if constexpr (OUT == PF_OUT_RESIDUAL) {
        const int64_t yplane = (b / y_div) * g.C + c;
        const float* __restrict__ yp = y + yplane * g.H * g.W;
        float racc = 0.f;
        for (int t = 0; t < T; ++t) {
            const int h = h0 + t;
            // every element is read and rewritten by the one thread that owns it
            for (int q = threadIdx.x; q < N; q += kBlock) {
                float gv = 0.f;
                float2* rp = res + t * NP + phase_slot(q);
                if (h < g.H && q < g.W) {
                    SP_DCHECK(h * g.W + q < g.H * g.W);
                    const float r = yp[h * g.W + q] - rp->x;
                    racc += r * r;
                    gv = gs * r;
                }
                *rp = make_float2(gv, 0.f);
            }
        }
        const float tsum = block_sum(racc, red);  // its barrier also orders the rewritten rows
        if (threadIdx.x == 0) partial[b * P + blockIdx.x] = tsum;
        __syncthreads();
        const float2* f = phase_fft(res, res == A ? B : A, tw, N, NP, T, false);
        for (int idx = threadIdx.x; idx < total; idx += kBlock) {
            const int kw = idx / T, t = idx - kw * T, h = h0 + t;
            if (h < g.H) {
                SP_DCHECK(kw < g.HW && kw * g.H + h < g.HW * g.H);
                wp[kw * g.H + h] = f[t * NP + phase_slot(kw)];
            }
        }
    } else if constexpr (OUT == PF_OUT_PROX || OUT == PF_OUT_PROX_ADD || OUT == PF_OUT_SCALE) {
        // z = the real part; four columns per thread (W % 4 == 0 for every transform length), so
        // x, xi and the output move as float4 and one Philox draw serves its four elements
        float* __restrict__ op_out = out + plane * g.H * g.W;
        const float* __restrict__ xp =
            px.step_form || OUT == PF_OUT_PROX_ADD ? px.x + plane * g.H * g.W : nullptr;
        const float* __restrict__ nzp = px.xi ? px.xi + plane * g.H * g.W : nullptr;
        const float inv_k = px.step_form ? 1.f / px.c.k : 1.f;
        const int groups = g.W / 4;
        SP_DCHECK(g.W % 4 == 0 && N == g.W);
        for (int idx = threadIdx.x; idx < T * groups; idx += kBlock) {
            const int t = idx / groups, j = (idx - t * groups) * 4, h = h0 + t;
            if (h >= g.H) continue;
            SP_DCHECK(h * g.W + j + 4 <= g.H * g.W);
            const float2* rl = res + t * NP;
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = rl[phase_slot(j + e)].x;
            if constexpr (OUT == PF_OUT_SCALE) {
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] *= gs;
            }
            if constexpr (OUT == PF_OUT_PROX_ADD) {
                float x0[4];
                load_v<4>(xp + h * g.W + j, x0);
                if (px.step_form) {  // the x0 of launch 1
                    float ev[4];
                    load_v<4>(px.eps + plane * g.H * g.W + h * g.W + j, ev);
#pragma unroll
                    for (int e = 0; e < 4; ++e) x0[e] = (x0[e] - px.c.k * ev[e]) / px.c.a;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] += x0[e];
            }
            if (px.step_form) {
                const int64_t el = (int64_t)c * g.H * g.W + h * g.W + j;  // flat element index
                float xv[4], nz[4];
                load_v<4>(xp + h * g.W + j, xv);
                if (nzp) load_v<4>(nzp + h * g.W + j, nz);
                else philox_normals<4>(px.seed, px.step, px.sample_offset + b, el, nz);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma clang fp contract(off)  // the bits of the expression as written, in both noise forms
                    o[e] = diffpir_update(px.c, inv_k, xv[e], o[e], nz[e]);
                }
            }
            store_v<4>(op_out + h * g.W + j, o);
        }
    } else {
        float* __restrict__ op_out = out + plane * g.H * g.W;
        for (int t = 0; t < T; ++t) {
            const int h = h0 + t;
            if (h >= g.H) break;
            const float2* rl = res + t * NP;
            for (int j = threadIdx.x; j < g.W; j += kBlock) {
                SP_DCHECK(h * g.W + j < g.H * g.W);
                float val;
                if constexpr (OUT == PF_OUT_AT) {
                    int lo, hi;
                    pf_images(j, g.R, g.W, g.mode, lo, hi);
                    SP_DCHECK(g.R + j < N && lo < g.R &&
                              (hi < 0 || (hi >= g.W + g.R && hi < g.W + 2 * g.R)));
                    val = rl[phase_slot(g.R + j)].x;
                    if (lo >= 0) val += rl[phase_slot(lo)].x;
                    if (hi >= 0) val += rl[phase_slot(hi)].x;
                } else {
                    val = rl[phase_slot(j)].x;
                }
                op_out[h * g.W + j] = val;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// The DDRM step of SP_OP_PSF_PERIODIC (samplers_hip.h): the right singular basis is the 2-D DFT,
// so x0, eps and the noise plane xi are transformed, combined per frequency and transformed back.
// Three launches through three intermediates of the layout above, `stride` float2 apart:
//   k_pf_rows_ddrm   row transforms of x0 = (x - k eps) / a, eps and xi (read, or drawn by Philox
//                    at the flat element index while staging) -> ws[0], ws[1], ws[2];
//   k_pf_cols_ddrm   per column tile the three forward column transforms, accumulated in registers
//                    as F = (f_th X0 + f_eps E + f_xi Xi) / (H W) + f_y q, one inverse column
//                    transform -> ws[0];
//   k_pf_rows_inv<PF_OUT_SCALE>  inverse rows, a_prev times the real part -> x'.
// A frequency is observed where P != 0, with s^2 = |M|^2; the class and the four coefficients are
// ddrm_class_coefs' (sp_ops.h).  Bytes per element: 12 (x, eps read, x' written; + 4 with xi
// injected) and the intermediates, (W / 2 + 1) / W * 8 B each: three written and read, one written
// and read again, + 8 of q and 16 of M and P per stored frequency (the spectra are shared by the
// batch).  Roundings of the longest path besides the transforms' own (4 log2 of each length,
// three forward and one inverse pair): x0 (4), s^2 (3), f_th (5: sp2, the product, r's three,
// 1 - r counted with them), its product with 1 / (H W) and with X0 (2), three sums (3), a_prev (1).
// ---------------------------------------------------------------------------
template <bool XI_IN>
__global__ __launch_bounds__(kBlock) void k_pf_rows_ddrm(pf_geom g, const float* __restrict__ x,
                                                         const float* __restrict__ eps,
                                                         const float* __restrict__ xi, uint64_t seed,
                                                         int64_t step, int64_t sample_offset, float a,
                                                         float k, float2* __restrict__ ws,
                                                         int64_t stride, int T) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int N = g.Nw, NP = phase_np(N);
    float2* tw = reinterpret_cast<float2*>(smem);
    float2* A = tw + N;
    float2* B = A + T * NP;
    const int tiles = (g.H + T - 1) / T, per = g.C * tiles;
    const int src = static_cast<int>(blockIdx.x) / per;  // 0: x0, 1: eps, 2: xi
    const int rem = static_cast<int>(blockIdx.x) - src * per;
    const int c = rem / tiles, h0 = (rem - c * tiles) * T;
    const int64_t b = blockIdx.y, plane = b * g.C + c;
    SP_DCHECK(src < 3 && c < g.C && h0 < g.H && N == g.W && g.W % 4 == 0);
    const int64_t base = plane * g.H * g.W;
    const float inv_a = 1.f / a;

    phase_twiddles(tw, N);
    const int groups = N / 4;
    for (int idx = threadIdx.x; idx < T * groups; idx += kBlock) {
        const int t = idx / groups, j = (idx - t * groups) * 4, h = h0 + t;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (h < g.H) {
            SP_DCHECK(h * g.W + j + 4 <= g.H * g.W);
            const int64_t off = base + h * g.W + j;
            if (src == 0) {
                float ev[4];
                load_v<4>(x + off, v);
                load_v<4>(eps + off, ev);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma clang fp contract(off)
                    v[e] = (v[e] - k * ev[e]) * inv_a;
                }
            } else if (src == 1) {
                load_v<4>(eps + off, v);
            } else if constexpr (XI_IN) {
                load_v<4>(xi + off, v);
            } else {
                philox_normals<4>(seed, step, sample_offset + b, off - b * g.C * g.H * g.W, v);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) A[t * NP + phase_slot(j + e)] = make_float2(v[e], 0.f);
    }
    __syncthreads();
    const float2* res = phase_fft(A, B, tw, N, NP, T, false);
    float2* __restrict__ wp = ws + src * stride + plane * (int64_t)g.HW * g.H;
    const int total = T * g.HW;
    for (int idx = threadIdx.x; idx < total; idx += kBlock) {
        const int kw = idx / T, t = idx - kw * T, h = h0 + t;
        if (h < g.H) {
            SP_DCHECK(kw < g.HW && kw * g.H + h < g.HW * g.H);
            wp[kw * g.H + h] = res[t * NP + phase_slot(kw)];
        }
    }
}

constexpr int kDdrmAcc = 8;  // frequencies of a column tile per thread: T * N <= 2000 < 8 * kBlock

__global__ __launch_bounds__(kBlock) void k_pf_cols_ddrm(pf_geom g, float2* __restrict__ ws,
                                                         int64_t stride, int T,
                                                         const float2* __restrict__ qs, int64_t y_div,
                                                         sp_ddrm_coefs cf) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int N = g.Nh, NP = phase_np(N);
    float2* tw = reinterpret_cast<float2*>(smem);
    float2* A = tw + N;
    float2* B = A + T * NP;
    const int tiles = (g.HW + T - 1) / T;
    const int c = static_cast<int>(blockIdx.x) / tiles;
    const int kw0 = (static_cast<int>(blockIdx.x) - c * tiles) * T;
    const int64_t plane = (int64_t)blockIdx.y * g.C + c;
    const int lines = min(T, g.HW - kw0), total = lines * N;
    SP_DCHECK(c < g.C && kw0 < g.HW && N == g.H && total <= kDdrmAcc * kBlock);
    const int64_t col0 = (plane * g.HW + kw0) * (int64_t)g.H;  // the tile's columns
    const float2* __restrict__ msp = g.spec + (int64_t)kw0 * N;              // M
    const float2* __restrict__ psp = msp + (int64_t)g.HW * N;                // P
    const int64_t qplane = ((int64_t)blockIdx.y / y_div) * g.C + c;
    const float2* __restrict__ qp = qs + (qplane * g.HW + kw0) * (int64_t)N;
    const float sc = 1.f / ((float)g.Nh * (float)g.Nw);

    phase_twiddles(tw, N);
    float2 acc[kDdrmAcc];
    float fth[kDdrmAcc], fep[kDdrmAcc], fxi[kDdrmAcc];
#pragma unroll
    for (int i = 0; i < kDdrmAcc; ++i) {
#pragma clang fp contract(off)
        const int idx = threadIdx.x + i * kBlock;
        acc[i] = make_float2(0.f, 0.f);
        fth[i] = fep[i] = fxi[i] = 0.f;
        if (idx < total) {
            const float2 m = msp[idx], pv = psp[idx], qv = qp[idx];
            const float s2 = m.x * m.x + m.y * m.y;
            const ddrm_f f = ddrm_class_coefs(cf, s2, pv.x != 0.f || pv.y != 0.f);
            fth[i] = f.th * sc, fep[i] = f.ep * sc, fxi[i] = f.xi * sc;
            acc[i] = make_float2(f.y * qv.x, f.y * qv.y);
        }
    }
    for (int src = 0; src < 3; ++src) {
        const float2* __restrict__ wp = ws + src * stride + col0;
        if (src) __syncthreads();  // the last transform's result is read before A is staged again
        for (int t = 0; t < T; ++t)
            for (int q = threadIdx.x; q < N; q += kBlock) {
                float2 val = make_float2(0.f, 0.f);
                if (t < lines) {
                    SP_DCHECK(q < g.H);
                    val = wp[t * g.H + q];
                }
                A[t * NP + phase_slot(q)] = val;
            }
        __syncthreads();
        const float2* z = phase_fft(A, B, tw, N, NP, T, false);
#pragma unroll
        for (int i = 0; i < kDdrmAcc; ++i) {
#pragma clang fp contract(off)
            const int idx = threadIdx.x + i * kBlock;
            if (idx < total) {
                const int t = idx / N, kh = idx - t * N;
                const float2 v = z[t * NP + phase_slot(kh)];
                const float f = src == 0 ? fth[i] : src == 1 ? fep[i] : fxi[i];
                acc[i] = make_float2(acc[i].x + f * v.x, acc[i].y + f * v.y);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kDdrmAcc; ++i) {
        const int idx = threadIdx.x + i * kBlock;
        if (idx < total) {
            const int t = idx / N, kh = idx - t * N;
            A[t * NP + phase_slot(kh)] = acc[i];
        }
    }
    __syncthreads();
    const float2* u = phase_fft(A, B, tw, N, NP, T, true);
    float2* __restrict__ w0 = ws + col0;
    const int keep = lines * g.H;
    for (int idx = threadIdx.x; idx < keep; idx += kBlock) {
        const int t = idx / g.H, h = idx - t * g.H;
        w0[idx] = u[t * NP + phase_slot(h)];
    }
}

// ---------------------------------------------------------------------------
// SP_OP_SR_PERIODIC: periodic blur-and-decimate super-resolution (operators/sr_periodic.py, pinned
// in fp64 by tests/sr_periodic_ops.py).  With s = op.factor, S the lattice [::s, ::s] and up = S^T
// (zero insertion), on exact-size transforms (Nh = H, Nw = W) as the periodic kind:
//   A x     = S IFFT2(FFT2(x) M)          A^T y = IFFT2(FFT2(up y) conj(M))
//   A^+T x  = S IFFT2(FFT2(x) conj(P))    A^+ y = IFFT2(FFT2(up y) P)
// Down (A, A^+T): k_pf_rows on the H rows, k_srp_cols<false> (stores the H / s lattice rows alone,
// compacted to the head of each column), k_srp_rows_inv<false> (transforms those rows, stores the
// W / s lattice columns).  Up (A^T, A^+): k_srp_rows_up (reads the (H / s) x (W / s) input,
// transforms the lattice rows alone), k_srp_cols<true> (inserts the zero rows in LDS),
// k_pf_rows_inv<PF_OUT_A>.  No launch reads, transforms or writes a row that is identically zero.
// The fused passes are down, then k_srp_rows_inv<true> on the lattice rows (g = gs (y - A x0), its
// r^2 partial, g zero-inserted along the row and transformed forward again), then up with
// conj(M) (DPS), P (PGDM) or conj(M) / (Lambda_t + rho) (prox), then the full inverse rows.
// Every sample alone, lines assigned by plane and tile, block_sum's fixed order, plain stores.
// ---------------------------------------------------------------------------
// launch 2.  UP false: H values a column in, the lattice rows h = s i out at [i], i < H / s.
// UP true: H / s values in from [i], placed at s i of a zero column, H values out.  Between the
// transforms times spec (conj_sign -1: its conjugate) / (H W); PROX: and / (Lambda_t + rho).
template <bool UP, bool PROX>
__global__ __launch_bounds__(kBlock) void k_srp_cols(pf_geom g, float2* __restrict__ ws, int T,
                                                     float conj_sign, float rho) {
    static_assert(UP || !PROX, "the prox multiplier belongs to the up launch");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int N = g.H, NP = phase_np(N);
    float2* tw = reinterpret_cast<float2*>(smem);
    float2* A = tw + N;
    float2* B = A + T * NP;
    const int tiles = (g.HW + T - 1) / T;
    const int c = static_cast<int>(blockIdx.x) / tiles;
    const int kw0 = (static_cast<int>(blockIdx.x) - c * tiles) * T;
    const int64_t plane = (int64_t)blockIdx.y * g.C + c;
    const int sh = __ffs(g.s) - 1, Hl = g.H >> sh;
    SP_DCHECK(c < g.C && kw0 < g.HW && N == g.Nh && g.s == (1 << sh) && (Hl << sh) == g.H);
    float2* __restrict__ wp = ws + (plane * g.HW + kw0) * (int64_t)g.H;  // the tile's columns
    const int lines = min(T, g.HW - kw0);

    phase_twiddles(tw, N);
    for (int t = 0; t < T; ++t)
        for (int q = threadIdx.x; q < N; q += kBlock) {
            float2 val = make_float2(0.f, 0.f);
            if (t < lines && (!UP || (q & (g.s - 1)) == 0)) {
                const int h = UP ? q >> sh : q;
                SP_DCHECK(h < (UP ? Hl : g.H));
                val = wp[t * g.H + h];
            }
            A[t * NP + phase_slot(q)] = val;
        }
    __syncthreads();
    float2* z = phase_fft(A, B, tw, N, NP, T, false);

    const float sc = 1.f / ((float)g.H * (float)g.W);
    const float2* __restrict__ hsp = g.spec + (int64_t)kw0 * N;
    const float* __restrict__ lam = PROX ? g.lam + (int64_t)kw0 * N : nullptr;
    const int total = lines * N;
    for (int idx = threadIdx.x; idx < total; idx += kBlock) {
        const int t = idx / N, kh = idx - t * N;
        SP_DCHECK(t < lines && kw0 + t < g.HW && kh < g.H);
        float2 m = hsp[idx];
        float f = sc;
        if constexpr (PROX) f = sc / (lam[idx] + rho);
        m.x *= f;
        m.y *= conj_sign * f;
        float2* zp = z + t * NP + phase_slot(kh);
        *zp = cmul(*zp, m);
    }
    __syncthreads();
    const float2* u = phase_fft(z, z == A ? B : A, tw, N, NP, T, true);
    const int rows = UP ? g.H : Hl, keep = lines * rows;
    for (int idx = threadIdx.x; idx < keep; idx += kBlock) {
        const int t = idx / rows, i = idx - t * rows, h = UP ? i : i << sh;
        SP_DCHECK(t < lines && h < g.H && t * g.H + i < lines * g.H);
        wp[t * g.H + i] = u[t * NP + phase_slot(h)];
    }
}

// launch 1 of the up maps: T rows of the (H / s) x (W / s) input, each zero-inserted onto the
// lattice columns, W-point FFT, the half spectrum stored transposed at [kw][i], i < H / s
__global__ __launch_bounds__(kBlock) void k_srp_rows_up(pf_geom g, const float* __restrict__ in,
                                                        float2* __restrict__ ws, int T) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int N = g.W, NP = phase_np(N);
    float2* tw = reinterpret_cast<float2*>(smem);
    float2* A = tw + N;
    float2* B = A + T * NP;
    const int sh = __ffs(g.s) - 1, Hl = g.H >> sh, Wl = g.W >> sh;
    const int tiles = (Hl + T - 1) / T;
    const int c = static_cast<int>(blockIdx.x) / tiles;
    const int i0 = (static_cast<int>(blockIdx.x) - c * tiles) * T;
    const int64_t plane = (int64_t)blockIdx.y * g.C + c;
    SP_DCHECK(c < g.C && i0 < Hl && N == g.Nw && g.s == (1 << sh) && (Wl << sh) == g.W);
    const float* __restrict__ ip = in + plane * Hl * Wl;

    phase_twiddles(tw, N);
    for (int t = 0; t < T; ++t) {
        const int i = i0 + t;
        for (int q = threadIdx.x; q < N; q += kBlock) {
            float val = 0.f;
            if (i < Hl && (q & (g.s - 1)) == 0) {
                SP_DCHECK((q >> sh) < Wl && i * Wl + (q >> sh) < Hl * Wl);
                val = ip[i * Wl + (q >> sh)];
            }
            A[t * NP + phase_slot(q)] = make_float2(val, 0.f);
        }
    }
    __syncthreads();
    const float2* res = phase_fft(A, B, tw, N, NP, T, false);
    float2* __restrict__ wp = ws + plane * (int64_t)g.HW * g.H;
    const int total = T * g.HW;
    for (int idx = threadIdx.x; idx < total; idx += kBlock) {
        const int kw = idx / T, t = idx - kw * T, i = i0 + t;
        if (i < Hl) {
            SP_DCHECK(kw < g.HW && kw * g.H + i < g.HW * g.H);
            wp[kw * g.H + i] = res[t * NP + phase_slot(kw)];
        }
    }
}

// launch 3 of the down maps on the H / s lattice rows at [kw][i].  RESIDUAL false: inverse FFT, the
// W / s lattice columns -> out.  True, the fused launch: g = gs (y - A x0) on the lattice and the
// r^2 partial of the tile (partial null: not stored), g zero-inserted along the row, forward FFT
// back to [kw][i].  y rows are y_stride floats apart.
template <bool RESIDUAL>
__global__ __launch_bounds__(kBlock) void k_srp_rows_inv(pf_geom g, float2* __restrict__ ws,
                                                         float* __restrict__ out,
                                                         const float* __restrict__ y, int64_t y_stride,
                                                         int64_t y_div, float gs,
                                                         float* __restrict__ partial, int P, int T,
                                                         const sp_step_rec* __restrict__ sched,
                                                         const int32_t* __restrict__ cursor) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float red[4];
    if (RESIDUAL && sched) gs = sched[*cursor].c.grad_scale;
    const int N = g.W, NP = phase_np(N);
    float2* tw = reinterpret_cast<float2*>(smem);
    float2* A = tw + N;
    float2* B = A + T * NP;
    const int sh = __ffs(g.s) - 1, Hl = g.H >> sh, Wl = g.W >> sh;
    const int tiles = (Hl + T - 1) / T;
    const int c = static_cast<int>(blockIdx.x) / tiles;
    const int i0 = (static_cast<int>(blockIdx.x) - c * tiles) * T;
    const int64_t b = blockIdx.y;
    const int64_t plane = b * g.C + c;
    SP_DCHECK(c < g.C && i0 < Hl && N == g.Nw && g.s == (1 << sh) &&
              (!RESIDUAL || static_cast<int>(blockIdx.x) < P));
    float2* __restrict__ wp = ws + plane * (int64_t)g.HW * g.H;

    phase_twiddles(tw, N);
    const int total = T * g.HW;
    for (int idx = threadIdx.x; idx < total; idx += kBlock) {
        const int kw = idx / T, t = idx - kw * T, i = i0 + t;
        float2 val = make_float2(0.f, 0.f);
        if (i < Hl) {
            SP_DCHECK(kw < g.HW && kw * g.H + i < g.HW * g.H);
            val = wp[kw * g.H + i];
        }
        A[t * NP + phase_slot(kw)] = val;
        if (kw > 0 && 2 * kw < N) {  // the spectrum of a real row: X[N - kw] = conj(X[kw])
            SP_DCHECK(N - kw >= g.HW && N - kw < N);
            A[t * NP + phase_slot(N - kw)] = make_float2(val.x, -val.y);
        }
    }
    __syncthreads();
    float2* res = phase_fft(A, B, tw, N, NP, T, true);

    if constexpr (RESIDUAL) {
        const float* __restrict__ yp = y + (b / y_div) * y_stride + (int64_t)c * Hl * Wl;
        float racc = 0.f;
        for (int t = 0; t < T; ++t) {
            const int i = i0 + t;
            // every element is read and rewritten by the one thread that owns it
            for (int q = threadIdx.x; q < N; q += kBlock) {
                float gv = 0.f;
                float2* rp = res + t * NP + phase_slot(q);
                if (i < Hl && (q & (g.s - 1)) == 0) {
                    SP_DCHECK((q >> sh) < Wl && i * Wl + (q >> sh) < Hl * Wl);
                    const float r = yp[i * Wl + (q >> sh)] - rp->x;
                    racc += r * r;
                    gv = gs * r;
                }
                *rp = make_float2(gv, 0.f);
            }
        }
        const float tsum = block_sum(racc, red);  // its barrier also orders the rewritten rows
        if (partial && threadIdx.x == 0) partial[b * P + blockIdx.x] = tsum;
        __syncthreads();
        const float2* f = phase_fft(res, res == A ? B : A, tw, N, NP, T, false);
        for (int idx = threadIdx.x; idx < total; idx += kBlock) {
            const int kw = idx / T, t = idx - kw * T, i = i0 + t;
            if (i < Hl) {
                SP_DCHECK(kw < g.HW && kw * g.H + i < g.HW * g.H);
                wp[kw * g.H + i] = f[t * NP + phase_slot(kw)];
            }
        }
    } else {
        float* __restrict__ op_out = out + plane * Hl * Wl;
        for (int t = 0; t < T; ++t) {
            const int i = i0 + t;
            if (i >= Hl) break;
            const float2* rl = res + t * NP;
            for (int j = threadIdx.x; j < Wl; j += kBlock) {
                SP_DCHECK(i * Wl + j < Hl * Wl && (j << sh) < N);
                op_out[i * Wl + j] = rl[phase_slot(j << sh)].x;
            }
        }
    }
}

// q of the prepares: row r of y (m floats) to q + r * stride
__global__ __launch_bounds__(kBlock) void k_srp_stash(const float* __restrict__ y,
                                                      float* __restrict__ q, int64_t m,
                                                      int64_t stride) {
    const int64_t r = blockIdx.y;
    SP_DCHECK(m <= stride);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock)
        q[r * stride + i] = y[r * m + i];
}

// ---------------------------------------------------------------------------
// host side (called from the entry points in sp_dps.hip; `op` is valid)
// ---------------------------------------------------------------------------
// SP_OP_PSF_PERIODIC is the wrap-around correlation on an image whose own sizes are transform
// lengths (Nh = H, Nw = W).  The blur is then exactly diagonal in the transform the kernels
// compute: A = IFFT2 M FFT2 with M = conj(FFT2(h centred at [0, 0])), so nothing is extended or
// folded, A^T has the multiplier conj(M), and the pseudo-inverse truncated to the kept frequencies
// has P = kept ? 1 / M : 0 (operators/periodic.py; both computed in fp64 by the caller).
// op.taps = M then P, each (re, im) pairs [W / 2 + 1][H].
//
// Both kinds run one pipeline: a pf_run (the entry point's name and timing kind, the geometry, the
// kernels' EXT) and the three stages pf_rows, pf_cols, pf_rows_inv / pf_rows_residual, which pick
// the kernel instantiation and go through fft_stage (sp_fft.h).  PSF_FFT has EXT = true on pf_size
// transforms (but for the row stage of A^T, which stages the rows as they are), PSF_PERIODIC
// EXT = false on exact-size ones with the multiplier M or P; pf_map and
// psf_fft_dps_residual are the only launch sequences of the maps and of DPS pass 1.  Every pass
// starts with pf_rows, which carries a timed pass's work (the batch); the later stages carry 0.
bool psf_fft_valid(const sp_op* op) {  // radius = R, factor = padding mode, taps = the spectrum
    if (!op->taps || op->keep_bits || op->word_rank || op->factor < 0 || op->factor > 2 ||
        op->channels <= 0 || op->height <= 0 || op->width <= 0 || op->radius < 1 ||
        op->radius > std::min(op->height, op->width) - 1 || op->height > 1024 || op->width > 1024 ||
        op->height + 2 * op->radius > 1024 || op->width + 2 * op->radius > 1024)
        return false;
    return (int64_t)op->channels * op->height * op->width == op->n && op->m == op->n &&
           phase_size_ok(pf_size(op->height + 2 * op->radius)) &&
           phase_size_ok(pf_size(op->width + 2 * op->radius));
}

bool psf_periodic_valid(const sp_op* op) {  // radius = R, factor = 0, taps = M then P
    if (!op->taps || op->keep_bits || op->word_rank || op->factor != 0 || op->channels <= 0 ||
        !phase_size_ok(op->height) || !phase_size_ok(op->width) || op->radius < 1 ||
        op->radius > (std::min(op->height, op->width) - 1) / 2)  // 2R + 1 <= min(H, W)
        return false;
    return (int64_t)op->channels * op->height * op->width == op->n && op->m == op->n;
}

enum { PP_SPEC_M = 0, PP_SPEC_P = 1 };  // the periodic kind's multipliers in op.taps

static inline bool pf_extends(const sp_op* op) { return op->kind == SP_OP_PSF_FFT; }

// `which`: the multiplier of the periodic kind; PSF_FFT has the one spectrum
static pf_geom pf_geometry(const sp_op* op, int which = PP_SPEC_M) {
    const bool ext = pf_extends(op);
    pf_geom g;
    g.C = op->channels, g.H = op->height, g.W = op->width, g.R = op->radius;
    g.mode = ext ? op->factor : PF_CIRCULAR;
    g.Nh = ext ? pf_size(op->height + 2 * op->radius) : op->height;
    g.Nw = ext ? pf_size(op->width + 2 * op->radius) : op->width;
    g.HW = g.Nw / 2 + 1;
    g.spec = reinterpret_cast<const float2*>(op->taps) + (int64_t)which * g.HW * g.Nh;
    const bool srp = op->kind == SP_OP_SR_PERIODIC;  // M, P, then Lambda_t
    g.s = srp ? op->factor : 1;
    g.lam = srp ? op->taps + 4 * (int64_t)g.HW * g.Nh : nullptr;
    return g;
}

static inline int pf_row_tiles(const pf_geom& g) {
    const int T = phase_lines(g.Nw);
    return (g.H + T - 1) / T;
}
static inline int pf_col_tiles(const pf_geom& g) {
    const int T = phase_lines(g.Nh);
    return (g.HW + T - 1) / T;
}

// row tiles per sample = workgroups per sample of the fused launch = r^2 partials per sample
int64_t psf_fft_partials(const sp_op* op) {
    return (int64_t)op->channels * pf_row_tiles(pf_geometry(op));
}

// floats of the intermediate
int64_t psf_fft_workspace(const sp_op* op, int64_t batch) {
    const pf_geom g = pf_geometry(op);
    return 2 * batch * g.C * (int64_t)g.HW * g.H;
}

struct pf_run {  // one entry point's pass of `batch` samples through the intermediate `ws`
    const char* what;
    int kind;  // timing kind, 0: untimed
    pf_geom g;
    bool ext;
    int64_t batch;
    float2* ws;
    hipStream_t s;
};

static pf_run pf_begin(const char* what, int kind, const sp_op* op, int which, int64_t batch,
                       float* work, hipStream_t s) {
    return {what, kind, pf_geometry(op, which), pf_extends(op), batch,
            reinterpret_cast<float2*>(work), s};
}

struct pf_x0 {  // the DPS form of the row stage: x0 = (in - k eps) / a, or sched[*cursor]'s a, k
    const float* eps;
    float a, k;
    const sp_step_rec* sched;
    const int32_t* cursor;
};

// launch 1: in (x0 of in, eps) -> ws; the rows are extended for A where the kind extends, and
// staged as they are for A^T (adj)
static int pf_rows(const pf_run& p, bool adj, const float* in, const pf_x0* x0 = nullptr) {
    const pf_geom& g = p.g;
    const pf_x0 f = x0 ? *x0 : pf_x0{kNoIn, 1.f, 0.f, kNoSched, kNoCursor};
    const bool ext = p.ext && !adj;
    const auto kern = x0 ? (ext ? k_pf_rows<true, true> : k_pf_rows<true, false>)
                         : (ext ? k_pf_rows<false, true> : k_pf_rows<false, false>);
    return fft_stage(p.what, p.kind, p.kind ? (double)p.batch : 0.0, kern, g.C * pf_row_tiles(g),
                     p.batch, g.Nw, p.s, g, in, f.eps, f.a, f.k, p.ws, phase_lines(g.Nw), f.sched,
                     f.cursor);
}

// launch 2 on ws: A or A^T (adj) of the map, or a form of the periodic kind with its arguments
static int pf_cols(const pf_run& p, bool adj, int form = PF_COL_MAP, const float2* qs = nullptr,
                   int64_t y_div = 1, float gs = 0.f) {
    const pf_geom& g = p.g;
    const auto kern = form == PF_COL_PREPARE ? (adj ? k_pf_cols<true, false, PF_COL_PREPARE>
                                                    : k_pf_cols<false, false, PF_COL_PREPARE>)
                      : form == PF_COL_PGDM  ? k_pf_cols<false, false, PF_COL_PGDM>
                      : form == PF_COL_PROX  ? k_pf_cols<false, false, PF_COL_PROX>
                      : p.ext                ? (adj ? k_pf_cols<true> : k_pf_cols<false>)
                                             : (adj ? k_pf_cols<true, false> : k_pf_cols<false, false>);
    return fft_stage(p.what, p.kind, 0.0, kern, g.C * pf_col_tiles(g), p.batch, g.Nh, p.s, g, p.ws,
                     phase_lines(g.Nh), qs, y_div, gs);
}

// launch 3: ws -> out, folded where the kind extends and the map is A^T
static int pf_rows_inv(const pf_run& p, bool adj, float* out) {
    const pf_geom& g = p.g;
    const auto kern = adj && p.ext ? k_pf_rows_inv<PF_OUT_AT> : k_pf_rows_inv<PF_OUT_A>;
    return fft_stage(p.what, p.kind, 0.0, kern, g.C * pf_row_tiles(g), p.batch, g.Nw, p.s, g, p.ws,
                     out, kNoIn, (int64_t)1, 0.f, kNoOut, 0, phase_lines(g.Nw), kNoSched, kNoCursor,
                     pf_prox_tail{});
}

// launch 3 of the proximal map: ws -> z, or the DiffPIR sample formed from z in the epilogue
static int pf_rows_prox(const pf_run& p, float* out, const pf_prox_tail& px, bool add_x0 = false) {
    const pf_geom& g = p.g;
    const auto kern = add_x0 ? k_pf_rows_inv<PF_OUT_PROX_ADD> : k_pf_rows_inv<PF_OUT_PROX>;
    return fft_stage(p.what, p.kind, 0.0, kern, g.C * pf_row_tiles(g), p.batch,
                     g.Nw, p.s, g, p.ws, out, kNoIn, (int64_t)1, 0.f, kNoOut, 0, phase_lines(g.Nw),
                     kNoSched, kNoCursor, px);
}

// the fused launch 3 + 1 of DPS pass 1: ws, r.y -> ws, r.partial
static int pf_rows_residual(const pf_run& p, const dps_residual_args& r) {
    const pf_geom& g = p.g;
    const int P = g.C * pf_row_tiles(g);
    return fft_stage(p.what, p.kind, 0.0, k_pf_rows_inv<PF_OUT_RESIDUAL>, P, p.batch, g.Nw, p.s, g,
                     p.ws, kNoOut, r.y, r.y_div, r.gs, r.partial, P, phase_lines(g.Nw), r.sched,
                     r.cursor, pf_prox_tail{});
}

// rows, columns, rows^-1 of the map with p's spectrum or of its transpose (adj): in -> ws -> out
static int pf_map(const pf_run& p, bool adj, const float* in, float* out) {
    int rc = pf_rows(p, adj, in);
    if (rc == SP_OK) rc = pf_cols(p, adj);
    if (rc == SP_OK) rc = pf_rows_inv(p, adj, out);
    return rc;
}

int psf_fft_apply(const sp_op* op, const float* x, float* y, int64_t batch, float* work,
                  hipStream_t s) {
    return pf_map(pf_begin("sp_op_apply_ws", 0, op, PP_SPEC_M, batch, work, s), false, x, y);
}

// the map is linear: A^T gy, x is not read
int psf_fft_vjp(const sp_op* op, const float* x, const float* gy, float* dx, int64_t batch,
                float* work, hipStream_t s) {
    (void)x;
    return pf_map(pf_begin("sp_op_vjp_ws", 0, op, PP_SPEC_M, batch, work, s), true, gy, dx);
}

// A^+ (multiplier P) or its transpose (conj(P))
int psf_periodic_pinv(const sp_op* op, const float* y, float* x, int64_t batch, int transpose,
                      float* work, hipStream_t s) {
    return pf_map(pf_begin("sp_op_pinv_ws", 0, op, PP_SPEC_P, batch, work, s), transpose != 0, y, x);
}

// rows (x, eps -> work), columns A, rows^-1 + rows (work, y -> work, partials), columns A^T,
// rows^-1 A^T (work -> v)
int psf_fft_dps_residual(const sp_op* op, const dps_residual_args& r, hipStream_t s) {
    const pf_run p =
        pf_begin("sp_dps_residual_ws", TK_DPS_RESIDUAL, op, PP_SPEC_M, r.batch, r.work, s);
    const pf_x0 x0 = {r.eps, r.a, r.k, r.sched, r.cursor};
    int rc = pf_rows(p, false, r.x, &x0);
    if (rc == SP_OK) rc = pf_cols(p, false);
    if (rc == SP_OK) rc = pf_rows_residual(p, r);
    if (rc == SP_OK) rc = pf_cols(p, true);
    if (rc == SP_OK) rc = pf_rows_inv(p, true, r.v);
    return rc;
}

// Q = P * FFT2(y) / (H W) per observation row, in the intermediate's layout: rows, then the
// column launch that stops at the spectrum.  y is fixed across a sampler call's steps, so this
// runs once and every step's column launch reads Q instead of transforming y again.
int psf_periodic_pgdm_prepare(const sp_op* op, const float* y, int64_t rows_y, float* q,
                              hipStream_t s) {
    const pf_run p = pf_begin("sp_pgdm_prepare", 0, op, PP_SPEC_P, rows_y, q, s);
    const int rc = pf_rows(p, false, y);
    return rc == SP_OK ? pf_cols(p, false, PF_COL_PREPARE) : rc;
}

// v = gs (A^+ y - Pi x0): rows (x, eps -> work), columns (z <- gs (Q - kept z) between the
// transforms), rows^-1 (work -> v)
int psf_periodic_pgdm_residual(const sp_op* op, const float* x, const float* eps, const float* q,
                               int64_t batch, int64_t y_div, const sp_dps_coefs& c, float* v,
                               float* work, hipStream_t s) {
    const pf_run p = pf_begin("sp_pgdm_residual_ws", TK_DPS_RESIDUAL, op, PP_SPEC_P, batch, work, s);
    const pf_x0 x0 = {eps, c.a, c.k, kNoSched, kNoCursor};
    int rc = pf_rows(p, false, x, &x0);
    if (rc == SP_OK)
        rc = pf_cols(p, false, PF_COL_PGDM, reinterpret_cast<const float2*>(q), y_div, c.grad_scale);
    if (rc == SP_OK) rc = pf_rows_inv(p, false, v);
    return rc;
}

// Q = conj(M) * FFT2(y) / (H W): sp_pgdm_prepare's two launches with the map's own multiplier
// conjugated (the column launch of A^T that stops at the spectrum)
int psf_periodic_prox_prepare(const sp_op* op, const float* y, int64_t rows_y, float* q,
                              hipStream_t s) {
    const pf_run p = pf_begin("sp_prox_prepare", 0, op, PP_SPEC_M, rows_y, q, s);
    const int rc = pf_rows(p, false, y);
    return rc == SP_OK ? pf_cols(p, true, PF_COL_PREPARE) : rc;
}

// z = Re IFFT2((Q + rho X0) / (|M|^2 + rho)): rows (x0, or x and eps -> work), columns
// (PF_COL_PROX between the transforms), rows^-1 with the prox epilogue (work -> z or x')
int psf_periodic_prox(const sp_op* op, const prox_args& a, hipStream_t s) {
    const pf_run p = pf_begin(a.eps ? "sp_diffpir_step_ws" : "sp_op_prox_ws", 0, op, PP_SPEC_M,
                              a.batch, a.work, s);
    const pf_x0 x0 = {a.eps, a.c.a, a.c.k, kNoSched, kNoCursor};
    int rc = pf_rows(p, false, a.x, a.eps ? &x0 : nullptr);
    if (rc == SP_OK)
        rc = pf_cols(p, false, PF_COL_PROX, reinterpret_cast<const float2*>(a.q), a.y_div, a.c.rho);
    if (rc == SP_OK)
        rc = pf_rows_prox(p, a.out,
                          {a.x, a.xi, nullptr, a.seed, a.step, a.sample_offset, a.c, a.eps != nullptr});
    return rc;
}

// the DDRM step: three intermediates (x0, eps, xi), see k_pf_rows_ddrm
int64_t psf_periodic_ddrm_workspace(const sp_op* op, int64_t batch) {
    return 3 * psf_fft_workspace(op, batch);
}

int psf_periodic_ddrm(const sp_op* op, const ddrm_args& a, hipStream_t s) {
    const pf_run p = pf_begin("sp_ddrm_step_ws", 0, op, PP_SPEC_M, a.batch, a.work, s);
    const pf_geom& g = p.g;
    const int64_t stride = psf_fft_workspace(op, a.batch) / 2;  // float2 of one intermediate
    if ((int64_t)phase_lines(g.Nh) * g.Nh > (int64_t)kDdrmAcc * kBlock) return SP_EUNSUPPORTED;
    const auto rows = a.xi ? k_pf_rows_ddrm<true> : k_pf_rows_ddrm<false>;
    int rc = fft_stage(p.what, 0, 0.0, rows, 3 * g.C * pf_row_tiles(g), p.batch, g.Nw, s, g, a.x, a.eps,
                       a.xi, a.seed, a.step, a.sample_offset, a.c.a, a.c.k, p.ws, stride,
                       phase_lines(g.Nw));
    if (rc == SP_OK)
        rc = fft_stage(p.what, 0, 0.0, k_pf_cols_ddrm, g.C * pf_col_tiles(g), p.batch, g.Nh, s, g, p.ws,
                       stride, phase_lines(g.Nh), reinterpret_cast<const float2*>(a.q), a.y_div, a.c);
    if (rc == SP_OK)
        rc = fft_stage(p.what, 0, 0.0, k_pf_rows_inv<PF_OUT_SCALE>, g.C * pf_row_tiles(g), p.batch, g.Nw,
                       s, g, p.ws, a.out, kNoIn, (int64_t)1, a.c.a_prev, kNoOut, 0, phase_lines(g.Nw),
                       kNoSched, kNoCursor, pf_prox_tail{});
    return rc;
}

// ---------------------------------------------------------------------------
// SP_OP_SR_PERIODIC, host side
// ---------------------------------------------------------------------------
// radius = K taps per axis, factor = s, taps = M, P (half spectra) then Lambda_t
bool sr_periodic_valid(const sp_op* op) {
    const int s = op->factor;
    if (!op->taps || op->keep_bits || op->word_rank || (s != 2 && s != 4 && s != 8) ||
        op->channels <= 0 || !phase_size_ok(op->height) || !phase_size_ok(op->width) ||
        op->height % s || op->width % s || op->radius < s ||
        op->radius > std::min(op->height, op->width) || (op->radius - s) % 2)
        return false;
    return (int64_t)op->channels * op->height * op->width == op->n && op->m * s * s == op->n;
}

// lattice rows per workgroup of the launches that transform the H / s lattice rows alone
static inline int srp_lines(const pf_geom& g) { return std::min(phase_lines(g.W), g.H / g.s); }
static inline int srp_tiles(const pf_geom& g) {
    const int T = srp_lines(g);
    return (g.H / g.s + T - 1) / T;
}

// lattice-row tiles per sample = workgroups per sample of the fused launch = r^2 partials
int64_t sr_periodic_partials(const sp_op* op) {
    return (int64_t)op->channels * srp_tiles(pf_geometry(op));
}

// launch 2: down (A, A^+T) or up (A^T, A^+, prox) with p's spectrum, conjugated or not
static int srp_cols(const pf_run& p, bool up, bool conj, bool prox = false, float rho = 0.f) {
    const pf_geom& g = p.g;
    const auto kern = prox ? k_srp_cols<true, true> : up ? k_srp_cols<true, false> : k_srp_cols<false, false>;
    return fft_stage(p.what, p.kind, 0.0, kern, g.C * pf_col_tiles(g), p.batch, g.H, p.s, g, p.ws,
                     phase_lines(g.H), conj ? -1.f : 1.f, rho);
}

static int srp_rows_up(const pf_run& p, const float* in) {
    const pf_geom& g = p.g;
    return fft_stage(p.what, p.kind, p.kind ? (double)p.batch : 0.0, k_srp_rows_up, g.C * srp_tiles(g),
                     p.batch, g.W, p.s, g, in, p.ws, srp_lines(g));
}

static int srp_rows_inv(const pf_run& p, float* out) {
    const pf_geom& g = p.g;
    return fft_stage(p.what, p.kind, 0.0, k_srp_rows_inv<false>, g.C * srp_tiles(g), p.batch, g.W, p.s,
                     g, p.ws, out, kNoIn, (int64_t)0, (int64_t)1, 0.f, kNoOut, 0, srp_lines(g), kNoSched,
                     kNoCursor);
}

// the fused middle launch: y rows `y_stride` floats apart; partial may be null (PGDM, prox)
static int srp_rows_residual(const pf_run& p, const float* y, int64_t y_stride, int64_t y_div, float gs,
                             float* partial, const sp_step_rec* sched, const int32_t* cursor) {
    const pf_geom& g = p.g;
    const int P = g.C * srp_tiles(g);
    return fft_stage(p.what, p.kind, 0.0, k_srp_rows_inv<true>, P, p.batch, g.W, p.s, g, p.ws, kNoOut,
                     y, y_stride, y_div, gs, partial, P, srp_lines(g), sched, cursor);
}

int sr_periodic_apply(const sp_op* op, const float* x, float* y, int64_t batch, float* work,
                      hipStream_t s) {
    const pf_run p = pf_begin("sp_op_apply_ws", 0, op, PP_SPEC_M, batch, work, s);
    int rc = pf_rows(p, false, x);
    if (rc == SP_OK) rc = srp_cols(p, false, false);
    if (rc == SP_OK) rc = srp_rows_inv(p, y);
    return rc;
}

int sr_periodic_vjp(const sp_op* op, const float* x, const float* gy, float* dx, int64_t batch,
                    float* work, hipStream_t s) {
    (void)x;
    const pf_run p = pf_begin("sp_op_vjp_ws", 0, op, PP_SPEC_M, batch, work, s);
    int rc = srp_rows_up(p, gy);
    if (rc == SP_OK) rc = srp_cols(p, true, true);
    if (rc == SP_OK) rc = pf_rows_inv(p, false, dx);
    return rc;
}

// A^+ (up, P) or its transpose (down, conj(P))
int sr_periodic_pinv(const sp_op* op, const float* y, float* x, int64_t batch, int transpose,
                     float* work, hipStream_t s) {
    const pf_run p = pf_begin("sp_op_pinv_ws", 0, op, PP_SPEC_P, batch, work, s);
    int rc = transpose ? pf_rows(p, false, y) : srp_rows_up(p, y);
    if (rc == SP_OK) rc = srp_cols(p, !transpose, transpose != 0);
    if (rc == SP_OK) rc = transpose ? srp_rows_inv(p, x) : pf_rows_inv(p, false, x);
    return rc;
}

// the first three launches of every fused pass: x0 -> A x0 on the lattice -> FFT rows of
// up(gs (y - A x0)) in the intermediate
static int srp_residual_head(const pf_run& p, const float* x, const pf_x0* x0, const float* y,
                             int64_t y_stride, int64_t y_div, float gs, float* partial,
                             const sp_step_rec* sched, const int32_t* cursor) {
    int rc = pf_rows(p, false, x, x0);
    if (rc == SP_OK) rc = srp_cols(p, false, false);
    if (rc == SP_OK) rc = srp_rows_residual(p, y, y_stride, y_div, gs, partial, sched, cursor);
    return rc;
}

int sr_periodic_dps_residual(const sp_op* op, const dps_residual_args& r, hipStream_t s) {
    const pf_run p =
        pf_begin("sp_dps_residual_ws", TK_DPS_RESIDUAL, op, PP_SPEC_M, r.batch, r.work, s);
    const pf_x0 x0 = {r.eps, r.a, r.k, r.sched, r.cursor};
    int rc = srp_residual_head(p, r.x, &x0, r.y, op->m, r.y_div, r.gs, r.partial, r.sched, r.cursor);
    if (rc == SP_OK) rc = srp_cols(p, true, true);
    if (rc == SP_OK) rc = pf_rows_inv(p, false, r.v);
    return rc;
}

// q of both prepares: y itself, one row per observation at the intermediate's per-sample stride
// (the callers size and slice q by sp_op_workspace(op, 1)).  The fused passes subtract A x0 on
// the lattice, where y is m floats a row; a spectrum of up(y) would be 2 s^2 times that to read.
static int srp_stash(const char* what, const sp_op* op, const float* y, int64_t rows, float* q,
                     hipStream_t s) {
    launch(0, k_srp_stash, dim3((unsigned)std::min<int64_t>(cdiv(op->m, kBlock), 1024), (unsigned)rows),
           dim3(kBlock), s, y, q, op->m, psf_fft_workspace(op, 1));
    return check_launch(what);
}

int sr_periodic_pgdm_prepare(const sp_op* op, const float* y, int64_t rows, float* q, hipStream_t s) {
    return srp_stash("sp_pgdm_prepare", op, y, rows, q, s);
}

int sr_periodic_prox_prepare(const sp_op* op, const float* y, int64_t rows, float* q, hipStream_t s) {
    return srp_stash("sp_prox_prepare", op, y, rows, q, s);
}

// v = gs A^+ (y - A x0): the DPS sequence with P in the second column launch
int sr_periodic_pgdm_residual(const sp_op* op, const float* x, const float* eps, const float* q,
                              int64_t batch, int64_t y_div, const sp_dps_coefs& c, float* v,
                              float* work, hipStream_t s) {
    const pf_run pm = pf_begin("sp_pgdm_residual_ws", TK_DPS_RESIDUAL, op, PP_SPEC_M, batch, work, s);
    const pf_run pp = pf_begin("sp_pgdm_residual_ws", TK_DPS_RESIDUAL, op, PP_SPEC_P, batch, work, s);
    const pf_x0 x0 = {eps, c.a, c.k, kNoSched, kNoCursor};
    int rc = srp_residual_head(pm, x, &x0, q, psf_fft_workspace(op, 1), y_div, c.grad_scale, kNoOut,
                               kNoSched, kNoCursor);
    if (rc == SP_OK) rc = srp_cols(pp, true, false);
    if (rc == SP_OK) rc = pf_rows_inv(pp, false, v);
    return rc;
}

// z = x0 + A^T (A A^T + rho)^-1 (y - A x0): the DPS sequence with conj(M) / (Lambda_t + rho) in
// the second column launch (every frequency divided), x0 added by the epilogue
int sr_periodic_prox(const sp_op* op, const prox_args& a, hipStream_t s) {
    const pf_run p = pf_begin(a.eps ? "sp_diffpir_step_ws" : "sp_op_prox_ws", 0, op, PP_SPEC_M,
                              a.batch, a.work, s);
    const pf_x0 x0 = {a.eps, a.c.a, a.c.k, kNoSched, kNoCursor};
    int rc = srp_residual_head(p, a.x, a.eps ? &x0 : nullptr, a.q, psf_fft_workspace(op, 1), a.y_div,
                               1.f, kNoOut, kNoSched, kNoCursor);
    if (rc == SP_OK) rc = srp_cols(p, true, true, true, a.c.rho);
    if (rc == SP_OK)
        rc = pf_rows_prox(p, a.out,
                          {a.x, a.xi, a.eps, a.seed, a.step, a.sample_offset, a.c, a.eps != nullptr},
                          true);
    return rc;
}

}  // namespace sp
