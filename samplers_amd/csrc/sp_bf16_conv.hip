// The bf16 priors' convolution (layout rationale and the MFMA's C layout: sp_bf16.h):
//
//   k_conv3x3_bf16<TC>   3x3 / stride 1 / padding 1 convolution (+ fp32 bias, + bf16 residual)
//                        and, with the flipped / transposed weight pack, its input VJP
//   k_conv_reduce        the fixed-order sum of a split-K launch's fp32 parts
//   k_pool2x2_bf16       Upsample2D's VJP

#define SP_TU 14  // debug-build site numbering (sp_common.h SP_DCHECK)
#include "sp_bf16.h"

namespace sp {

#ifndef SP_CONV_XCD
#define SP_CONV_XCD 1  // XCD-aware workgroup order of the bf16 conv tile (k_conv3x3_bf16)
#endif
constexpr bool kConvXcdRemap = SP_CONV_XCD != 0;

// ---------------------------------------------------------------------------------------------
// 3x3 convolution, NHWC, implicit GEMM on v_mfma_f32_32x32x16_bf16.
//
// Workgroup: 64 output channels x 512 output pixels, 4 waves; wave w holds all 64 channels of
// pixels 128 w .. 128 w + 127 (2 x 4 MFMA tiles of 32 x 32: channels as A rows, pixels as B
// columns, 128 accumulators).  The 512 pixels are TR "virtual rows" of TC columns: TC = 32 for
// W % 32 == 0 (16 image rows of one sample), TC = W = H for the 16 / 8 / 4 levels (S whole
// samples per tile, each with its own zero halo rows).  The contraction is staged 16 input
// channels at a time: the weights of the stage ([tap][64 co][16 ci]) and the input patch
// ([S (SR + 2) rows][TC + 2 cols][16 ci], zero halo) go to LDS as 48-byte rows (32 bytes + 16
// pad: the 16 lanes of a ds_read_b128 group then read 16 distinct 4-bank slots for any start
// pixel), 9 taps x 8 MFMAs per wave per stage; the next stage's global loads are issued into
// registers before the current stage's MFMAs.
// ---------------------------------------------------------------------------------------------
#ifndef SP_CONV_PRIO
#define SP_CONV_PRIO 0  // wave priority around the TC = 32 pipeline's phases (A/B knob, 0 = none)
#endif

// threadIdx.x re-read opaque to the compiler: the shortcut stages' per-thread addresses are then
// formed inside their loop instead of being hoisted ahead of the 3x3 loop (where they were live
// across it: the kernel spilled ~200 VGPRs)
__device__ __forceinline__ int cv_tid() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

template <int TC>
struct CvGeo {
    static_assert(TC == 32 || TC == 16 || TC == 8 || TC == 4, "tile width");
    static constexpr int PX = 512;
    static constexpr int TR = PX / TC;                // virtual rows per tile
    static constexpr int SR = TC == 32 ? 16 : TC;     // image rows per sample segment
    static constexpr int S = TR / SR;                 // sample segments per tile
    static constexpr int PW = TC + 2;                 // patch columns
    static constexpr int PH = S * (SR + 2);           // patch rows
    static constexpr int PQ = PH * PW;                // patch pixels
    // TC = 32: 32-byte rows with the two 16-byte halves swapped on every other group of 8 rows
    // (weights) / 8 columns (patch) — conflict-free for the fragment reads — and two stage
    // buffers; else 48-byte rows (32 bytes + 16 pad), one buffer
    static constexpr bool DB = TC == 32;
    static constexpr int RB = DB ? 32 : 48;           // LDS bytes per row
    static constexpr int WROWS = 9 * 64;              // weight rows per stage
    static constexpr int LW = WROWS * RB;
    static constexpr int LP = PQ * RB;
    static constexpr int BUF = LW + LP;               // one stage
    static constexpr int LDS = DB ? 2 * BUF : BUF;
    static constexpr int NW = (WROWS * 2 + kBlock - 1) / kBlock;  // 16-byte weight pieces per thread
    static constexpr int PQP = PQ;
    static constexpr int NP = (PQP * 2 + kBlock - 1) / kBlock;    // 16-byte patch pieces per thread
};

// 16-byte piece p of an LDS image of 32-byte rows (48-byte stride): row p / 2, chunk p % 2 —
// consecutive lanes read the two halves of a pixel's 32 bytes (measured faster than writing one
// chunk of 64 rows per instruction, which avoids the 2-way ds_write conflicts but doubles the
// cache lines each global load instruction touches: -8 % on the 64x64 / 512x512 layers)
__device__ __forceinline__ int cv_row(int p) { return p >> 1; }
__device__ __forceinline__ int cv_chunk(int p) { return p & 1; }

// UP: the input is the half-resolution tensor of diffusers' Upsample2D and the patch reads
// pixel (h >> 1, w >> 1) of it for full-resolution pixel (h, w): conv(upsample_nearest2x(x))
// without the upsampled tensor in HBM.
// part != NULL (split-K, gridDim.z parts over the input-channel stages): part z of the
// contraction is stored as fp32 to part[z][n h w][cout] without bias / residual (k_conv_reduce).
// SC (TC = 32): a 1x1 convolution of cat(xs1, xs2) (cs1 + cs2 channels, NHWC, the ResnetBlock's
// conv_shortcut) is summed into the same accumulators as (cs1 + cs2) / 16 further stages of the
// contraction — weights wsp [co block of 64][cs / 16][64 co][16 ci], the stage's 512 pixels
// written to the patch centre and read by the centre tap only (8 MFMAs per wave) — so the
// shortcut's output is never written to HBM nor read back as a residual.
// GS (TC = 32, unsplit): the output y is the cotangent dz of a GroupNorm(+SiLU) over cat(gx1, gx2)
// (gc1 + gc2 = cout channels, NHWC) and the epilogue also emits that GroupNorm VJP's per-(tile,
// channel) sums sum(g), sum(g xhat) (g = dz act'(y) gamma) over the tile's 512 pixels, from dz as
// stored (bf16) and the per-(n, c) coefficients gco = [sc | sh | xs | xo] (k_gnb_coefs): gpart
// [n][tile][2][cout], tile = the tile's index within its sample — the layout k_gnb_final_bwd
// reads, so the separate sums pass (x and dz read again) is not run.
// FS (TC = 32, unsplit): the output y feeds a GroupNorm over y + cb (cb = gn.co: per-(n, c) fp32
// or NULL) and the epilogue emits its per-(tile, channel) shifted moments from y as stored:
// gpart [n][tile][3][cout] = sum(d), sum(d^2), K with d = y + cb - K and K the tile's first pixel's
// y + cb (k_gnb_final_fwd_tiles) — the forward statistics pass is not run.
template <int TC, bool UP, bool BLK = false, bool SC = false, bool GS = false, bool FS = false>
__global__ __launch_bounds__(kBlock, TC == 4 ? 1 : 2) void k_conv3x3_bf16(const u16* __restrict__ x, const u16* __restrict__ wp,
                                                         const float* __restrict__ bias, const u16* __restrict__ res,
                                                         int n, int cin, int cout, int h, int w,
                                                         u16* __restrict__ y, float* __restrict__ part,
                                                         const u16* __restrict__ xs1, const u16* __restrict__ xs2,
                                                         int cs1, int cs2, const u16* __restrict__ wsp, ConvGn gn) {
    static_assert(!SC || (TC == 32 && !UP), "shortcut stages: TC = 32 tiles");
    static_assert(!GS || (TC == 32 && !UP && !SC), "GroupNorm VJP sums: TC = 32 tiles");
    static_assert(!FS || (TC == 32 && !UP && !GS), "GroupNorm moments: TC = 32 tiles");
    using G = CvGeo<TC>;
    __shared__ __attribute__((aligned(16))) char lds[G::LDS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, hh = lane >> 5;
    // XCD-aware order: the hardware deals workgroups to the 8 XCDs round-robin by dispatch order,
    // which would put the output-channel blocks of one pixel tile (consecutive ids, cb fastest)
    // on 8 different L2s, each fetching the same patch; remapped, XCD x runs ids x T/8 ..
    // (x + 1) T/8 - 1 in order, so a tile's channel blocks and its neighbours share one L2
    int cb = blockIdx.x, pt = blockIdx.y;
    if (kConvXcdRemap) {  // (the blur kernels' mapping: XCD x gets ceil / floor(nb / 8) ids)
        const unsigned nb = gridDim.x * gridDim.y, lin = blockIdx.x + gridDim.x * blockIdx.y;
        const unsigned q8 = nb / 8, r8 = nb % 8, xcd = lin % 8, loc = lin / 8;
        const unsigned l2 = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + loc;
        cb = static_cast<int>(l2 % gridDim.x), pt = static_cast<int>(l2 / gridDim.x);
    }
    int n0, h0, c0;
    if constexpr (TC == 32) {
        const int strips = w >> 5, rowblk = h / G::SR;
        c0 = (pt % strips) * 32;
        const int t = pt / strips;
        h0 = (t % rowblk) * G::SR;
        n0 = t / rowblk;
    } else {
        c0 = 0, h0 = 0, n0 = pt * G::S;
    }
    const int nci = cin >> 4, nsc = SC ? (cs1 + cs2) >> 4 : 0;
    const bq_u4* __restrict__ wsrc = reinterpret_cast<const bq_u4*>(wp + (int64_t)cb * nci * (9 * 64 * 16));

    // per-thread patch pieces: global element offset (channel 0 of the stage) or -1 (halo / past the batch)
    int64_t poff[G::NP];
#pragma unroll
    for (int k = 0; k < G::NP; ++k) {
        const int i = tid + k * kBlock;
        poff[k] = -1;
        if (i < 2 * G::PQP && cv_row(i) < G::PQ) {
            const int q = cv_row(i), half = cv_chunk(i);
            const int prow = q / G::PW, pcol = q - prow * G::PW;
            const int seg = prow / (G::SR + 2), pr = prow - seg * (G::SR + 2);
            const int nn = n0 + seg, hi = h0 + pr - 1, wi = c0 + pcol - 1;
            if (nn < n && (unsigned)hi < (unsigned)h && (unsigned)wi < (unsigned)w) {
                if constexpr (UP)
                    poff[k] = (((int64_t)nn * (h >> 1) + (hi >> 1)) * (w >> 1) + (wi >> 1)) * cin + half * 8;
                else if constexpr (BLK)  // [n][cin / 16][h][w][16]: stage ks is plane ks of the sample
                    poff[k] = ((int64_t)nn * (cin >> 4) * h * w + (int64_t)hi * w + wi) * 16 + half * 8;
                else
                    poff[k] = (((int64_t)nn * h + hi) * w + wi) * cin + half * 8;
            }
        }
    }
    bq_u4 sw[G::NW], spx[G::NP];
    const int64_t kstride = BLK ? (int64_t)h * w * 16 : 16;  // elements between stages' pieces
    // shortcut stage k1: the 64 x 16 weights (threads < 128, one piece each) and the tile's 512
    // pixels x 16 channels of cat(xs1, xs2) (4 pieces per thread; TC = 32 tiles lie inside the image)
    auto gload_sc = [&](int k1) {
        const int tid = cv_tid();
        if (tid < 128) sw[0] = reinterpret_cast<const bq_u4*>(wsp)[((int64_t)cb * nsc + k1) * 128 + tid];
        // piece k of thread tid: pixel (tid / 2) + 128 k = row (tid / 64) + 4 k, column (tid / 2) % 32
        const bool first = k1 * 16 < cs1;
        const int64_t cstr = first ? cs1 : cs2;
        const int q0 = tid >> 1;
        const u16* __restrict__ src = (first ? xs1 + k1 * 16 : xs2 + (k1 * 16 - cs1)) + (tid & 1) * 8 +
                                      (((int64_t)n0 * h + h0 + (q0 >> 5)) * w + c0 + (q0 & 31)) * cstr;
        const int64_t kstep = 4 * (int64_t)w * cstr;
#pragma unroll
        for (int k = 0; k < 4; ++k) spx[k] = *reinterpret_cast<const bq_u4*>(src + k * kstep);
    };
    auto gload = [&](int ks) {
        const bq_u4* __restrict__ ws = wsrc + (int64_t)ks * (9 * 64 * 2);
#pragma unroll
        for (int k = 0; k < G::NW; ++k) {
            const int i = tid + k * kBlock;
            if (i < G::WROWS * 2) sw[k] = ws[2 * cv_row(i) + cv_chunk(i)];
        }
#pragma unroll
        for (int k = 0; k < G::NP; ++k)
#if BQ_EXP == 10  // diagnostics (wrong results): every patch piece from one cached 32-byte line per stage
            spx[k] = poff[k] >= 0 ? *reinterpret_cast<const bq_u4*>(x + (tid & 1) * 8 + ks * 16) : bq_u4{0u, 0u, 0u, 0u};
#else
            spx[k] = poff[k] >= 0 ? *reinterpret_cast<const bq_u4*>(x + poff[k] + ks * kstride) : bq_u4{0u, 0u, 0u, 0u};
#endif
    };
    auto lstore = [&]() {
#pragma unroll
        for (int k = 0; k < G::NW; ++k) {
            const int i = tid + k * kBlock;
            if (i < G::WROWS * 2) *reinterpret_cast<bq_u4*>(lds + cv_row(i) * G::RB + cv_chunk(i) * 16) = sw[k];
        }
#pragma unroll
        for (int k = 0; k < G::NP; ++k) {
            const int i = tid + k * kBlock;
            if (i < 2 * G::PQP && cv_row(i) < G::PQ)
                *reinterpret_cast<bq_u4*>(lds + G::LW + cv_row(i) * G::RB + cv_chunk(i) * 16) = spx[k];
        }
    };

    // B-operand base of each of the wave's 4 pixel tiles (tap (0, 0)); tap (dy, dx) adds dy PW + dx
    int qb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = 128 * wv + 32 * j + r, vr = p / TC, col = p - vr * TC;
        const int seg = vr / G::SR, rr = vr - seg * G::SR;
        qb[j] = ((seg * (G::SR + 2) + rr) * G::PW + col) * G::RB + hh * 16;
    }
    bq_f16 acc[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[a][j] = bq_f16{};

    const int kz = blockIdx.z, nz = gridDim.z, ntot = nci + nsc;
    const int ks0 = kz * ntot / nz, ks1 = (kz + 1) * ntot / nz;
    if constexpr (G::DB) {
        // Two stage buffers, one barrier per stage: stage s + 1 (in registers since stage s - 1)
        // is written to the other buffer and stage s + 2's global loads are issued before stage
        // s's MFMAs; the barrier after them both publishes stage s + 1 and frees stage s's buffer.
        // Swizzle: weight row wr keeps its 16-byte half c at (c ^ (wr >> 3 & 1)); patch pixel q
        // (column q % PW) at (c ^ (q % PW >> 3 & 1)) — the 16-lane groups of a ds_read_b128 then
        // read 16 distinct 16-byte slots of the 256-byte bank row for any column offset.
        auto lstore_sc = [&](int b) {  // the shortcut stage: weights as tap 0, pixels at the patch centre
            const int tid = cv_tid();
            char* __restrict__ base = lds + b * G::BUF;
            if (tid < 128) {
                const int wr = tid >> 1;
                *reinterpret_cast<bq_u4*>(base + wr * 32 + (((tid & 1) ^ ((wr >> 3) & 1)) << 4)) = sw[0];
            }
            const int q0 = tid >> 1, pcol = (q0 & 31) + 1;
            char* __restrict__ pp = base + G::LW + (((q0 >> 5) + 1) * G::PW + pcol) * 32 +
                                    (((tid & 1) ^ ((pcol >> 3) & 1)) << 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) *reinterpret_cast<bq_u4*>(pp + k * 4 * G::PW * 32) = spx[k];
        };
        auto lstore_db = [&](int b) {
            char* __restrict__ base = lds + b * G::BUF;
#pragma unroll
            for (int k = 0; k < G::NW; ++k) {
                const int i = tid + k * kBlock;
                if (i < G::WROWS * 2) {
                    const int wr = cv_row(i);
                    *reinterpret_cast<bq_u4*>(base + wr * 32 + ((cv_chunk(i) ^ ((wr >> 3) & 1)) << 4)) = sw[k];
                }
            }
#pragma unroll
            for (int k = 0; k < G::NP; ++k) {
                const int i = tid + k * kBlock;
                if (i < 2 * G::PQP && cv_row(i) < G::PQ) {
                    const int q = cv_row(i), col = q % G::PW;
                    *reinterpret_cast<bq_u4*>(base + G::LW + q * 32 + ((cv_chunk(i) ^ ((col >> 3) & 1)) << 4)) = spx[k];
                }
            }
        };
        // per-lane fragment offsets: A row 64 t + 32 a + r (its swizzle bit is r's); B pixel
        // (4 wv + i) PW + r + dx, column r + dx
        const int wl_lane = r * 32 + ((hh ^ ((r >> 3) & 1)) << 4);
        int bl_lane[3];
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) bl_lane[dx] = G::LW + (4 * wv * G::PW + r + dx) * 32 + ((hh ^ (((r + dx) >> 3) & 1)) << 4);
        auto compute = [&](int b) {
            const char* __restrict__ base = lds + b * G::BUF;
            bq_u4 fa[9][2], fb[3][6];
            auto lda = [&](int s) {
                const int dx = s / 3, dy = s - 3 * dx, t = 3 * dy + dx;
                fa[s][0] = *reinterpret_cast<const bq_u4*>(base + wl_lane + (t * 64) * 32);
                fa[s][1] = *reinterpret_cast<const bq_u4*>(base + wl_lane + (t * 64 + 32) * 32);
                if (dy == 0) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) fb[dx][i] = *reinterpret_cast<const bq_u4*>(base + bl_lane[dx] + i * G::PW * 32);
                } else {
                    fb[dx][dy + 3] = *reinterpret_cast<const bq_u4*>(base + bl_lane[dx] + (dy + 3) * G::PW * 32);
                }
            };
            lda(0);
#pragma unroll
            for (int s = 0; s < 9; ++s) {
#if BQ_EXP == 8  // diagnostics (wrong results): tap 0's fragments for every tap, no further LDS reads
                if (s + 1 < 9) {
                    const int dx1 = (s + 1) / 3, dy1 = (s + 1) - 3 * dx1;
                    fa[s + 1][0] = fa[0][0], fa[s + 1][1] = fa[0][1];
                    if (dy1 == 0) {
                        for (int i = 0; i < 4; ++i) fb[dx1][i] = fb[0][i];
                    } else {
                        fb[dx1][dy1 + 3] = fb[0][dy1 - 1];
                    }
                }
#else
                if (s + 1 < 9) lda(s + 1);
#endif
                const int dx = s / 3, dy = s - 3 * dx;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[0][j] = bq_mfma(fa[s][0], fb[dx][j + dy], acc[0][j]);
                    acc[1][j] = bq_mfma(fa[s][1], fb[dx][j + dy], acc[1][j]);
                }
                // issue order pinned: tap s + 1's fragment reads, then tap s's 8 MFMAs (left to
                // itself the scheduler sinks each read to just before its first use, so every
                // tap waited for its LDS latency behind a single MFMA: MFMA busy 0.52)
                if (s + 1 < 9) {
                    const int dx1 = (s + 1) / 3, dy1 = (s + 1) - 3 * dx1;
                    if (dy1 == 0) __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
                    else __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        // the shortcut stage's centre-tap MFMAs (fragments as compute's tap (1, 1))
        auto compute_sc = [&](int b) {
            const int t = cv_tid(), ln = t & 63, rr = ln & 31, h2 = ln >> 5, wq = t >> 6;
            const char* __restrict__ base = lds + b * G::BUF;
            const int wl = rr * 32 + ((h2 ^ ((rr >> 3) & 1)) << 4);
            const int bl = G::LW + (4 * wq * G::PW + rr + 1) * 32 + ((h2 ^ (((rr + 1) >> 3) & 1)) << 4);
            const bq_u4 a0 = *reinterpret_cast<const bq_u4*>(base + wl);
            const bq_u4 a1 = *reinterpret_cast<const bq_u4*>(base + wl + 32 * 32);
            bq_u4 f[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) f[j] = *reinterpret_cast<const bq_u4*>(base + bl + (j + 1) * G::PW * 32);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[0][j] = bq_mfma(a0, f[j], acc[0][j]);
                acc[1][j] = bq_mfma(a1, f[j], acc[1][j]);
            }
        };
        // stages kb .. ke - 1 through the two buffers (gl: global loads of a stage into registers,
        // st: registers -> LDS buffer, cp: the buffer's MFMAs); the shortcut's stages (part z's
        // share of stages nci ..) in a loop of their own ahead of the 3x3 stages (one loop over
        // both kinds, or the shortcut's loop second, spilled ~200 VGPRs)
        auto pipeline = [&](int kb, int ke, auto&& gl, auto&& st, auto&& cp) {
            const int nst = ke - kb;
            if (nst <= 0) return;
            gl(kb);
            st(0);
            if (nst > 1) gl(kb + 1);
            __syncthreads();
            for (int s = 0; s < nst; ++s) {
                const int b = s & 1;
#if SP_CONV_PRIO == 1  // A/B knob: the stage hand-off and next loads issued at raised priority
                __builtin_amdgcn_s_setprio(2);
#endif
                if (s + 1 < nst) st(b ^ 1);
#if BQ_EXP == 9  // diagnostics (wrong results): no global loads after the prologue's two stages
                (void)b;
#else
                if (s + 2 < nst) gl(kb + s + 2);
#endif
                __builtin_amdgcn_sched_barrier(0);
#if SP_CONV_PRIO == 1
                __builtin_amdgcn_s_setprio(0);
#elif SP_CONV_PRIO == 2  // A/B knob: the MFMA phase at raised priority
                __builtin_amdgcn_s_setprio(2);
#endif
                cp(b);
#if SP_CONV_PRIO == 2
                __builtin_amdgcn_s_setprio(0);
#endif
                __syncthreads();
            }
        };
        if constexpr (SC)
            pipeline(ks0 > nci ? ks0 - nci : 0, ks1 - nci, gload_sc, lstore_sc, compute_sc);
        pipeline(ks0, ks1 < nci ? ks1 : nci, gload, lstore_db, compute);
    } else {
        gload(ks0);
        for (int ks = ks0; ks < ks1; ++ks) {
            __syncthreads();  // the previous stage's fragment reads are done
            lstore();
            __syncthreads();
            if (ks + 1 < ks1) gload(ks + 1);
            const char* __restrict__ wl = lds + r * G::RB + hh * 16;
            const char* __restrict__ pl = lds + G::LW;
            // fragments of tap t + 1 are read while tap t's 8 MFMAs run (two register sets)
            bq_u4 fa[2][2], fb[2][4];
            auto frags = [&](int t, int slot) {
                const int dy = t / 3, dx = t - 3 * (t / 3);
                fa[slot][0] = *reinterpret_cast<const bq_u4*>(wl + (t * 64) * G::RB);
                fa[slot][1] = *reinterpret_cast<const bq_u4*>(wl + (t * 64 + 32) * G::RB);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    fb[slot][j] = *reinterpret_cast<const bq_u4*>(pl + qb[j] + (dy * G::PW + dx) * G::RB);
            };
            frags(0, 0);
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                if (t + 1 < 9) frags(t + 1, (t + 1) & 1);
                const int sl = t & 1;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[0][j] = bq_mfma(fa[sl][0], fb[sl][j], acc[0][j]);
                    acc[1][j] = bq_mfma(fa[sl][1], fb[sl][j], acc[1][j]);
                }
                // tap t + 1's 6 reads, then tap t's 8 MFMAs (as the TC = 32 loop; TC = 8 holds
                // 7 staged patch pieces per thread and would spill with both register sets live)
                if constexpr (TC != 8) {
                    if (t + 1 < 9) __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }

    // epilogue: lane (pixel r of tile j) holds channels 64 cb + 32 a + 8 g + 4 hh + e in register 4 g + e
    if constexpr (FS) {
        const float* __restrict__ cbp = gn.co;
        // the tile's first pixel (wave 0, j = 0, r = 0: lanes 0 / 32) as stored + cb: the shifts K
        float* kb = reinterpret_cast<float*>(lds) + 512;  // [64 local channels]
        if (wv == 0 && r == 0) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int cl = 32 * a + 8 * g + 4 * hh, co = cb * 64 + cl;
                    if (co >= cout) continue;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float t = acc[a][0][4 * g + e];
                        if (bias) t += bias[co + e];
                        if (res) t += bf1(res[(((int64_t)n0 * h + h0) * w + c0) * cout + co + e]);
                        kb[cl + e] = bf1(f2bf(t)) + (cbp ? cbp[(int64_t)n0 * cout + co + e] : 0.f);
                    }
                }
        }
        __syncthreads();
        float V[64];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int cl = 32 * a + 8 * g + 4 * hh, co = cb * 64 + cl;
                const bool live = co < cout;  // cout % 16 == 0
                float K[4], C[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) K[e] = live ? kb[cl + e] : 0.f;
                if (live && cbp) {
                    const float4 c4 = *reinterpret_cast<const float4*>(cbp + (int64_t)n0 * cout + co);
                    C[0] = c4.x, C[1] = c4.y, C[2] = c4.z, C[3] = c4.w;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (!live) continue;
                    const int64_t obase = (((int64_t)n0 * h + h0 + 4 * wv + j) * w + c0 + r) * cout;
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc[a][j][4 * g + e];
                    if (bias) {
                        const float4 bb = *reinterpret_cast<const float4*>(bias + co);
                        v[0] += bb.x, v[1] += bb.y, v[2] += bb.z, v[3] += bb.w;
                    }
                    if (res) {
                        const bq_u2 rv = *reinterpret_cast<const bq_u2*>(res + obase + co);
                        v[0] += bf_lo(rv.x), v[1] += bf_hi(rv.x), v[2] += bf_lo(rv.y), v[3] += bf_hi(rv.y);
                    }
                    const bq_u2 yv{pk2(v[0], v[1]), pk2(v[2], v[3])};
                    *reinterpret_cast<bq_u2*>(y + obase + co) = yv;
                    const float yf[4] = {bf_lo(yv.x), bf_hi(yv.x), bf_lo(yv.y), bf_hi(yv.y)};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {  // the terms of k_gnb_stats<0, _> with the tile's shift
                        const float d = yf[e] + C[e] - K[e];
                        s1[e] += d;
                        s2[e] = fmaf(d, d, s2[e]);
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) V[2 * ((a * 4 + g) * 4 + e)] = s1[e], V[2 * ((a * 4 + g) * 4 + e) + 1] = s2[e];
            }
#pragma unroll
        for (int m = 16, L = 64; m >= 1; m >>= 1, L >>= 1) {  // halving exchanges, as the GS epilogue
            const bool up = (r & m) != 0;
#pragma unroll
            for (int k = 0; k < L / 2; ++k) {
                const float keep = up ? V[L / 2 + k] : V[k], give = up ? V[k] : V[L / 2 + k];
                V[k] = keep + __shfl_xor(give, m, 64);
            }
        }
        float* red = reinterpret_cast<float*>(lds);  // [wave][stat][64 local channels] (kb lies past it)
        {
            const int i = r, a = i >> 4, g = (i >> 2) & 3, e = i & 3, cl = 32 * a + 8 * g + 4 * hh + e;
            red[(wv * 2 + 0) * 64 + cl] = V[0];
            red[(wv * 2 + 1) * 64 + cl] = V[1];
        }
        __syncthreads();
        if (tid < 192) {
            const int st = tid >> 6, cl = tid & 63, co = cb * 64 + cl;
            const float t = st == 2 ? kb[cl]
                                    : ((red[(0 * 2 + st) * 64 + cl] + red[(1 * 2 + st) * 64 + cl]) +
                                       red[(2 * 2 + st) * 64 + cl]) + red[(3 * 2 + st) * 64 + cl];
            const int tiles = (h / G::SR) * (w >> 5), tile = (h0 / G::SR) * (w >> 5) + (c0 >> 5);
            if (co < cout) gn.part[(((int64_t)n0 * tiles + tile) * 3 + st) * cout + co] = t;
        }
        return;
    }
    if constexpr (GS) {
        // dz stored, and per lane the sums over its 4 pixels (j) of each of its 32 channels: V[2 i + s],
        // i = (a 4 + g) 4 + e, s = 0: sum g, 1: sum g xhat
        const int64_t nc = (int64_t)n * cout;
        const int c2 = cout - gn.c1;
        // restrict-qualified: the x / coefficient loads may then be issued ahead of the dz stores
        // (unqualified, every load waited for the store before it)
        const u16* __restrict__ gx1 = gn.x1;
        const u16* __restrict__ gx2 = gn.x2;
        const float* __restrict__ gco = gn.co;
        const float* __restrict__ ggm = gn.gamma;
        float V[64];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co = cb * 64 + 32 * a + 8 * g + 4 * hh;
                const bool live = co < cout;  // cout % 16 == 0: a lane's 4 channels are all in or all out
                const int cl = live ? co : 0;
                const float4 k0 = *reinterpret_cast<const float4*>(gco + (int64_t)n0 * cout + cl);
                const float4 k1 = *reinterpret_cast<const float4*>(gco + nc + (int64_t)n0 * cout + cl);
                const float4 k2 = *reinterpret_cast<const float4*>(gco + 2 * nc + (int64_t)n0 * cout + cl);
                const float4 k3 = *reinterpret_cast<const float4*>(gco + 3 * nc + (int64_t)n0 * cout + cl);
                const float4 gm4 = ggm ? *reinterpret_cast<const float4*>(ggm + cl) : make_float4(1.f, 1.f, 1.f, 1.f);
                const float K0[4] = {k0.x, k0.y, k0.z, k0.w}, K1[4] = {k1.x, k1.y, k1.z, k1.w};
                const float K2[4] = {k2.x, k2.y, k2.z, k2.w}, K3[4] = {k3.x, k3.y, k3.z, k3.w};
                const float GM[4] = {gm4.x, gm4.y, gm4.z, gm4.w};
                float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
                bq_u2 xq[4];  // the 4 pixels' x, loaded before any of their arithmetic
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t pix = ((int64_t)n0 * h + h0 + 4 * wv + j) * w + c0 + r;
                    xq[j] = !live ? bq_u2{0u, 0u}
                          : co < gn.c1 ? *reinterpret_cast<const bq_u2*>(gx1 + pix * gn.c1 + co)
                                       : *reinterpret_cast<const bq_u2*>(gx2 + pix * c2 + (co - gn.c1));
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t pix = ((int64_t)n0 * h + h0 + 4 * wv + j) * w + c0 + r;
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc[a][j][4 * g + e];
                    if (!live) continue;
                    if (bias) {
                        const float4 bb = *reinterpret_cast<const float4*>(bias + co);
                        v[0] += bb.x, v[1] += bb.y, v[2] += bb.z, v[3] += bb.w;
                    }
                    const bq_u2 dzv{pk2(v[0], v[1]), pk2(v[2], v[3])};
                    *reinterpret_cast<bq_u2*>(y + pix * cout + co) = dzv;
                    const bq_u2 xv = xq[j];
                    const float xf[4] = {bf_lo(xv.x), bf_hi(xv.x), bf_lo(xv.y), bf_hi(xv.y)};
                    const float df[4] = {bf_lo(dzv.x), bf_hi(dzv.x), bf_lo(dzv.y), bf_hi(dzv.y)};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {  // the terms of k_gnb_stats<1, ACT>
                        const float yv = fmaf(xf[e], K0[e], K1[e]);
                        float d = df[e];
                        if (gn.act) {
                            const float sg = __builtin_amdgcn_rcpf(1.f + __expf(-yv));
                            d *= sg * (1.f + yv * (1.f - sg));
                        }
                        const float gg = d * GM[e];
                        s1[e] += gg;
                        s2[e] = fmaf(gg, fmaf(xf[e], K2[e], K3[e]), s2[e]);
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) V[2 * ((a * 4 + g) * 4 + e)] = s1[e], V[2 * ((a * 4 + g) * 4 + e) + 1] = s2[e];
            }
        // sum over the 32 lanes of each half-wave (its 32 pixels of each tile row) by halving
        // exchanges: after the step with mask m a lane keeps the half of its values selected by
        // its lane bit m; lane r ends with V[2 r], V[2 r + 1] = value index r's two sums
#pragma unroll
        for (int m = 16, L = 64; m >= 1; m >>= 1, L >>= 1) {
            const bool up = (r & m) != 0;
#pragma unroll
            for (int k = 0; k < L / 2; ++k) {
                const float keep = up ? V[L / 2 + k] : V[k], give = up ? V[k] : V[L / 2 + k];
                V[k] = keep + __shfl_xor(give, m, 64);
            }
        }
        __syncthreads();  // the stage buffers are free: the wave totals meet in LDS
        float* red = reinterpret_cast<float*>(lds);  // [wave][stat][64 local channels]
        {
            const int i = r, a = i >> 4, g = (i >> 2) & 3, e = i & 3, cl = 32 * a + 8 * g + 4 * hh + e;
            red[(wv * 2 + 0) * 64 + cl] = V[0];
            red[(wv * 2 + 1) * 64 + cl] = V[1];
        }
        __syncthreads();
        if (tid < 128) {
            const int st = tid >> 6, cl = tid & 63, co = cb * 64 + cl;
            const float t = ((red[(0 * 2 + st) * 64 + cl] + red[(1 * 2 + st) * 64 + cl]) + red[(2 * 2 + st) * 64 + cl]) +
                            red[(3 * 2 + st) * 64 + cl];
            const int tiles = (h / G::SR) * (w >> 5), tile = (h0 / G::SR) * (w >> 5) + (c0 >> 5);
            if (co < cout) gn.part[(((int64_t)n0 * tiles + tile) * 2 + st) * cout + co] = t;
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = 128 * wv + 32 * j + r, vr = p / TC, col = p - vr * TC;
        const int seg = vr / G::SR, rr = vr - seg * G::SR;
        const int nn = n0 + seg;
        if (nn >= n) continue;
        const int64_t obase = (((int64_t)nn * h + h0 + rr) * w + c0 + col) * cout;
        SP_DCHECK(h0 + rr < h && c0 + col < w);
        if (part) {  // split-K partial (cout % 4 == 0): fp32, no bias / residual
            float* pp = part + (int64_t)kz * ((int64_t)n * h * w * cout) + obase;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int co = cb * 64 + 32 * a + 8 * g + 4 * hh;
                    if (co + 4 <= cout)
                        *reinterpret_cast<float4*>(pp + co) = make_float4(acc[a][j][4 * g], acc[a][j][4 * g + 1],
                                                                          acc[a][j][4 * g + 2], acc[a][j][4 * g + 3]);
                }
            continue;
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co = cb * 64 + 32 * a + 8 * g + 4 * hh;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[a][j][4 * g + e];
                if (co + 4 <= cout && (cout & 3) == 0) {
                    if (bias) {
                        const float4 bb = *reinterpret_cast<const float4*>(bias + co);
                        v[0] += bb.x, v[1] += bb.y, v[2] += bb.z, v[3] += bb.w;
                    }
                    if (res) {
                        const bq_u2 rv = *reinterpret_cast<const bq_u2*>(res + obase + co);
                        v[0] += bf_lo(rv.x), v[1] += bf_hi(rv.x), v[2] += bf_lo(rv.y), v[3] += bf_hi(rv.y);
                    }
                    *reinterpret_cast<bq_u2*>(y + obase + co) = bq_u2{pk2(v[0], v[1]), pk2(v[2], v[3])};
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (co + e < cout) {
                            float t = v[e] + (bias ? bias[co + e] : 0.f);
                            if (res) t += bf1(res[obase + co + e]);
                            y[obase + co + e] = f2bf(t);
                        }
                }
            }
    }
}

static int conv_tc(int h, int w) {
    if (w % 32 == 0 && h % 16 == 0) return 32;
    if (h == w && (w == 16 || w == 8 || w == 4)) return w;
    return 0;
}

// y = sum over the split-K parts (fixed order) + bias (+ res), 4 channels per thread-iteration
__global__ __launch_bounds__(kBlock) void k_conv_reduce(const float* __restrict__ part, int parts, int64_t total,
                                                        int cout, const float* __restrict__ bias,
                                                        const u16* __restrict__ res, u16* __restrict__ y) {
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < total / 4; v += (int64_t)gridDim.x * kBlock) {
        const int64_t i = 4 * v;
        float4 a = *reinterpret_cast<const float4*>(part + i);
        for (int z = 1; z < parts; ++z) {
            const float4 b = *reinterpret_cast<const float4*>(part + (int64_t)z * total + i);
            a.x += b.x, a.y += b.y, a.z += b.z, a.w += b.w;
        }
        const int co = static_cast<int>(i % cout);
        if (bias) a.x += bias[co], a.y += bias[co + 1], a.z += bias[co + 2], a.w += bias[co + 3];
        if (res) {
            const bq_u2 rv = *reinterpret_cast<const bq_u2*>(res + i);
            a.x += bf_lo(rv.x), a.y += bf_hi(rv.x), a.z += bf_lo(rv.y), a.w += bf_hi(rv.y);
        }
        *reinterpret_cast<bq_u2*>(y + i) = bq_u2{pk2(a.x, a.y), pk2(a.z, a.w)};
    }
}

template <int TC>
static int64_t conv_tiles(int n, int h, int w) {
    using G = CvGeo<TC>;
    if constexpr (TC == 32)
        return (int64_t)n * (h / G::SR) * (w / 32);
    else
        return (n + G::S - 1) / G::S;
}

// split-K parts for a launch whose workgroups leave CUs idle (fewer than two per CU): doubling
// while each part keeps >= 8 input-channel stages and the grid stays under ~4 per CU
static int conv_parts(int n, int cin, int cout, int h, int w) {
    const int tc = conv_tc(h, w);
    if (!tc || cout % 4) return 1;
    const int64_t tiles = tc == 32 ? conv_tiles<32>(n, h, w) : tc == 16 ? conv_tiles<16>(n, h, w)
                        : tc == 8 ? conv_tiles<8>(n, h, w) : conv_tiles<4>(n, h, w);
    const int64_t wgs = tiles * ((cout + 63) / 64);
    int parts = 1;
    while (wgs * parts < 512 && (cin / 16) / (2 * parts) >= 8 && parts < 16) parts *= 2;
    return parts;
}

// the shortcut operands of an SC launch (wsp == nullptr: none)
struct ConvSc {
    const u16* xs1 = nullptr;
    const u16* xs2 = nullptr;
    int cs1 = 0, cs2 = 0;
    const u16* wsp = nullptr;
};

template <int TC, bool UP, bool BLK = false, bool SC = false, bool GS = false, bool FS = false>
static void conv_bf16_launch(const u16* x, const u16* wp, const float* bias, const u16* res, int n, int cin,
                             int cout, int h, int w, u16* y, hipStream_t s, float* part = nullptr, int parts = 1,
                             const ConvSc& sc = ConvSc{}, const ConvGn& gn = ConvGn{}) {
    using G = CvGeo<TC>;
    (void)sizeof(G);
    const int cbn = (cout + 63) / 64;
    const int64_t tiles = conv_tiles<TC>(n, h, w);
    // (+ the shortcut stages' 1x1 contraction)
    const double flops = 18.0 * n * (double)h * w * cin * cout + 2.0 * n * (double)h * w * (sc.cs1 + sc.cs2) * cout;
    launch_w(TK_CONV_BF16, flops, k_conv3x3_bf16<TC, UP, BLK, SC, GS, FS>, dim3(cbn, static_cast<unsigned>(tiles), parts),
             dim3(kBlock), s, x, wp, bias, res, n, cin, cout, h, w, y, parts > 1 ? part : nullptr, sc.xs1, sc.xs2,
             sc.cs1, sc.cs2, sc.wsp, gn);
    if (parts > 1) {
        const int64_t total = (int64_t)n * h * w * cout;
        launch(0, k_conv_reduce, dim3(stream_blocks(total / 8)), dim3(kBlock), s, static_cast<const float*>(part),
               parts, total, cout, bias, res, y);
    }
}

// the NHWC tile of the shape's width (conv_tc != 0)
template <bool UP>
static void conv_bf16_dispatch(const u16* x, const u16* wp, const float* bias, const u16* res, int n, int cin, int cout,
                               int h, int w, u16* y, hipStream_t s, float* part = nullptr, int parts = 1) {
    switch (conv_tc(h, w)) {
        case 32: conv_bf16_launch<32, UP>(x, wp, bias, res, n, cin, cout, h, w, y, s, part, parts); break;
        case 16: conv_bf16_launch<16, UP>(x, wp, bias, res, n, cin, cout, h, w, y, s, part, parts); break;
        case 8: conv_bf16_launch<8, UP>(x, wp, bias, res, n, cin, cout, h, w, y, s, part, parts); break;
        default: conv_bf16_launch<4, UP>(x, wp, bias, res, n, cin, cout, h, w, y, s, part, parts); break;
    }
}

// Upsample2D's VJP after the full-resolution input VJP: dx[n][i][j][c] = sum of the 2 x 2 block
// dz[n][2i + a][2j + b][c] (fp32 sum, one rounding), 8 channels per thread-iteration
__global__ __launch_bounds__(kBlock) void k_pool2x2_bf16(const u16* __restrict__ dz, int64_t n, int c, int hs, int ws,
                                                         u16* __restrict__ dx) {
    const int cv = c / 8;
    const int64_t total = n * hs * ws * cv;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < total; v += (int64_t)gridDim.x * kBlock) {
        const int j = static_cast<int>(v % cv);
        const int64_t pix = v / cv, nn = pix / ((int64_t)hs * ws), rem = pix - nn * hs * ws;
        const int i = static_cast<int>(rem / ws), jj = static_cast<int>(rem - (int64_t)i * ws);
        float acc[8] = {};
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                float f[8];
                unpack8(*reinterpret_cast<const bq_u4*>(
                            dz + (((nn * 2 * hs + 2 * i + a) * (2 * ws) + 2 * jj + b) * c + 8 * j)), f);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += f[e];
            }
        *reinterpret_cast<bq_u4*>(dx + pix * c + 8 * j) = pack8(acc);
    }
}

}  // namespace sp

using namespace sp;

extern "C" {

// ---- 3x3 convolution ------------------------------------------------------------------------

int sp_conv3x3_bf16_supported(int32_t cin, int32_t cout, int32_t h, int32_t w) {
    return cin > 0 && cin % 16 == 0 && cout > 0 && conv_tc(h, w) != 0;
}

// elements (bf16) of the packed weights: [ceil(cout/64)][cin/16][9][64][16]
int64_t sp_conv3x3_bf16_packed_size(int32_t cin, int32_t cout) {
    return (int64_t)((cout + 63) / 64) * 64 * cin * 9;
}

// y[n][h][w][cout] = conv3x3(x[n][h][w][cin], W) + bias (+ res), NHWC bf16, fp32 accumulation.
// wp: packed as [co block of 64][ci block of 16][tap 3 ky + kx][64 co][16 ci] (rows past cout
// zero); the input VJP is the same call with the pack of W'[ci][co][2-ky][2-kx].
static int conv_bf16_call(const void* x, const void* wp, const float* bias, const void* res, int64_t n, int32_t cin,
                          int32_t cout, int32_t h, int32_t w, void* y, sp_stream_t stream, bool up,
                          void* ws = nullptr, int64_t ws_bytes = 0, int blk = 0, const ConvSc& sc = ConvSc{}) {
    if (!x || !wp || !y || n <= 0 || !sp_conv3x3_bf16_supported(cin, cout, h, w)) return SP_EINVAL;
    if (blk && (up || conv_tc(h, w) != 32)) return SP_EINVAL;
    const int cs = sc.cs1 + sc.cs2;
    if (sc.wsp && (up || res || conv_tc(h, w) != 32 || !sc.xs1 || sc.cs1 <= 0 || sc.cs1 % 16 || sc.cs2 < 0 ||
                   sc.cs2 % 16 || (sc.cs2 && !sc.xs2) || n * h * (int64_t)w * cs >= (int64_t(1) << 40)))
        return SP_EINVAL;
    if (up && (h % 2 || w % 2)) return SP_EINVAL;
    if (n * h * (int64_t)w * std::max(cin, cout) >= (int64_t(1) << 40) || n >= (int64_t(1) << 30)) return SP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const u16* xx = static_cast<const u16*>(x);
    const u16* ww = static_cast<const u16*>(wp);
    const u16* rr = static_cast<const u16*>(res);
    u16* yy = static_cast<u16*>(y);
    const int ni = static_cast<int>(n);
    if (up) {
        conv_bf16_dispatch<true>(xx, ww, bias, rr, ni, cin, cout, h, w, yy, s);
        return check_launch("sp_conv3x3_bf16_up");
    }
    int parts = conv_parts(ni, cin + (sc.wsp ? cs : 0), cout, h, w);
    if (parts > 1 && (!ws || ws_bytes < 4 * parts * (int64_t)ni * h * w * cout)) parts = 1;
    float* part = static_cast<float*>(ws);
    if (sc.wsp) {
        if (blk) conv_bf16_launch<32, false, true, true>(xx, ww, bias, rr, ni, cin, cout, h, w, yy, s, part, parts, sc);
        else conv_bf16_launch<32, false, false, true>(xx, ww, bias, rr, ni, cin, cout, h, w, yy, s, part, parts, sc);
        return check_launch("sp_conv3x3_bf16_sc");
    }
    if (blk) {
        conv_bf16_launch<32, false, true>(xx, ww, bias, rr, ni, cin, cout, h, w, yy, s, part, parts);
        return check_launch("sp_conv3x3_bf16_ex");
    }
    conv_bf16_dispatch<false>(xx, ww, bias, rr, ni, cin, cout, h, w, yy, s, part, parts);
    return check_launch("sp_conv3x3_bf16");
}

// bytes of the split-K workspace sp_conv3x3_bf16_ws uses for this shape (0: the launch fills the
// chip unsplit): parts x n h w cout fp32
int64_t sp_conv3x3_bf16_workspace(int64_t n, int32_t cin, int32_t cout, int32_t h, int32_t w) {
    if (n <= 0 || n >= (int64_t(1) << 30) || !sp_conv3x3_bf16_supported(cin, cout, h, w)) return 0;
    const int parts = conv_parts(static_cast<int>(n), cin, cout, h, w);
    return parts > 1 ? 4 * parts * n * h * (int64_t)w * cout : 0;
}

// sp_conv3x3_bf16 with split-K over the input channels where the workgroups would leave CUs idle:
// the parts' fp32 sums go to ws (sp_conv3x3_bf16_workspace bytes) and a fixed-order reduce adds
// them with the bias / residual (deterministic); ws = NULL or short: unsplit
int sp_conv3x3_bf16_ws(const void* x, const void* wp, const float* bias, const void* res, int64_t n, int32_t cin,
                       int32_t cout, int32_t h, int32_t w, void* y, void* ws, int64_t ws_bytes, sp_stream_t stream) {
    return conv_bf16_call(x, wp, bias, res, n, cin, cout, h, w, y, stream, false, ws, ws_bytes);
}

// sp_conv3x3_bf16_ws with the input in a chosen layout: in_layout 0 = NHWC, 1 = channel-blocked
// [n][cin / 16][h][w][16] (each 16-channel stage of the tile reads whole lines; TC = 32 shapes only:
// sp_conv3x3_bf16_blk_supported).  The output stays NHWC.
int sp_conv3x3_bf16_blk_supported(int32_t cin, int32_t cout, int32_t h, int32_t w) {
    return sp_conv3x3_bf16_supported(cin, cout, h, w) && conv_tc(h, w) == 32;
}

int sp_conv3x3_bf16_ex(const void* x, int32_t in_layout, const void* wp, const float* bias, const void* res, int64_t n,
                       int32_t cin, int32_t cout, int32_t h, int32_t w, void* y, void* ws, int64_t ws_bytes,
                       sp_stream_t stream) {
    if (in_layout != 0 && in_layout != 1) return SP_EINVAL;
    return conv_bf16_call(x, wp, bias, res, n, cin, cout, h, w, y, stream, false, ws, ws_bytes, in_layout);
}

// y = conv3x3(x) + conv1x1(cat(xs1, xs2)) + bias: the ResnetBlock's conv2 with its conv_shortcut summed
// as further stages of the same contraction (no shortcut tensor, no residual read).  wsp: the 1x1
// weights packed as [co block of 64][cs / 16][64 co][16 ci] (sp_conv3x3_bf16_sc_packed_size
// elements, rows past cout zero); bias: conv2's + the shortcut's.  TC = 32 shapes
// (sp_conv3x3_bf16_sc_supported); split-K over all stages (sp_conv3x3_bf16_sc_workspace).
int sp_conv3x3_bf16_sc_supported(int32_t cin, int32_t cout, int32_t cs1, int32_t cs2, int32_t h, int32_t w) {
    return sp_conv3x3_bf16_supported(cin, cout, h, w) && conv_tc(h, w) == 32 && cs1 > 0 && cs1 % 16 == 0 &&
           cs2 >= 0 && cs2 % 16 == 0;
}

int64_t sp_conv3x3_bf16_sc_packed_size(int32_t cs, int32_t cout) { return (int64_t)((cout + 63) / 64) * 64 * cs; }

int64_t sp_conv3x3_bf16_sc_workspace(int64_t n, int32_t cin, int32_t cs, int32_t cout, int32_t h, int32_t w) {
    if (n <= 0 || n >= (int64_t(1) << 30) || cs < 0 || !sp_conv3x3_bf16_supported(cin, cout, h, w)) return 0;
    const int parts = conv_parts(static_cast<int>(n), cin + cs, cout, h, w);
    return parts > 1 ? 4 * parts * n * h * (int64_t)w * cout : 0;
}

int sp_conv3x3_bf16_sc(const void* x, int32_t in_layout, const void* wp, const float* bias, const void* xs1,
                       const void* xs2, int32_t cs1, int32_t cs2, const void* wsp, int64_t n, int32_t cin, int32_t cout,
                       int32_t h, int32_t w, void* y, void* ws, int64_t ws_bytes, sp_stream_t stream) {
    if ((in_layout != 0 && in_layout != 1) || !wsp || !sp_conv3x3_bf16_sc_supported(cin, cout, cs1, cs2, h, w))
        return SP_EINVAL;
    ConvSc sc;
    sc.xs1 = static_cast<const u16*>(xs1), sc.xs2 = static_cast<const u16*>(xs2);
    sc.cs1 = cs1, sc.cs2 = cs2, sc.wsp = static_cast<const u16*>(wsp);
    return conv_bf16_call(x, wp, bias, nullptr, n, cin, cout, h, w, y, stream, false, ws, ws_bytes, in_layout, sc);
}

int sp_conv3x3_bf16(const void* x, const void* wp, const float* bias, const void* res, int64_t n, int32_t cin,
                    int32_t cout, int32_t h, int32_t w, void* y, sp_stream_t stream) {
    return conv_bf16_call(x, wp, bias, res, n, cin, cout, h, w, y, stream, false);
}

// y = conv3x3(upsample_nearest2x(x)) + bias (+ res): x [n][h/2][w/2][cin], y [n][h][w][cout]
int sp_conv3x3_bf16_up(const void* x, const void* wp, const float* bias, const void* res, int64_t n, int32_t cin,
                       int32_t cout, int32_t h, int32_t w, void* y, sp_stream_t stream) {
    return conv_bf16_call(x, wp, bias, res, n, cin, cout, h, w, y, stream, true);
}

// dx[n][h/2][w/2][c] = 2 x 2 block sums of dz[n][h][w][c] (Upsample2D's VJP), NHWC bf16
int sp_pool2x2_bf16(const void* dz, int64_t n, int32_t c, int32_t h, int32_t w, void* dx, sp_stream_t stream) {
    if (!dz || !dx || n <= 0 || c <= 0 || c % 8 || h <= 0 || w <= 0 || h % 2 || w % 2) return SP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t vec = n * (h / 2) * (int64_t)(w / 2) * (c / 8);
    launch(0, k_pool2x2_bf16, dim3(stream_blocks(vec)), dim3(kBlock), s, static_cast<const u16*>(dz), n, c, h / 2,
           w / 2, static_cast<u16*>(dx));
    return check_launch("sp_pool2x2_bf16");
}

// ---- conv input VJP + the GroupNorm VJP it feeds, with the GroupNorm sums from the conv epilogue ----

static int64_t gnv_tiles(int32_t h, int32_t w) { return (int64_t)(h / 16) * (w / 32); }

int sp_conv3x3_bf16_gnvjp_supported(int64_t n, int32_t cin, int32_t cout, int32_t h, int32_t w, int32_t c1,
                                    int32_t groups) {
    return n > 0 && n <= 65535 && sp_conv3x3_bf16_supported(cin, cout, h, w) && conv_tc(h, w) == 32 &&
           cout % 16 == 0 && c1 > 0 && c1 % 16 == 0 && c1 <= cout &&
           sp_groupnorm_bf16_supported(c1, cout - c1, groups) &&
           conv_parts(static_cast<int>(n), cin, cout, h, w) == 1 &&
           n * h * (int64_t)w * std::max(cin, cout) < (int64_t(1) << 40);
}

// workspace bytes (fp32): per-tile sums [n][tiles][2][cout] + coefficients [4][n][cout] + [3][n][cout]
int64_t sp_conv3x3_bf16_gnvjp_workspace(int64_t n, int32_t cout, int32_t h, int32_t w) {
    return 4 * (n * gnv_tiles(h, w) * 2 * (int64_t)cout + 7 * n * (int64_t)cout);
}

// dz = conv3x3 input VJP of dy (the conv's flipped / transposed weight pack wp, dy in in_layout as
// sp_conv3x3_bf16_ex, cin = dy's channels, cout = dz's), then dx1 / dx2 = the input VJP of
// sp_groupnorm_bf16_fwd over cat(x1, x2) (c1 + c2 = cout channels) at dz, + the addends — as
// sp_conv3x3_bf16_ex followed by sp_groupnorm_bf16_bwd_ex, except that the GroupNorm VJP's sums
// come from the conv's epilogue (per 512-pixel tile, fixed order) instead of a pass that reads dz
// and x again.  dz: a caller buffer [n][h][w][cout] (written, then read by the apply pass).
int sp_conv3x3_bf16_gnvjp(const void* dy, int32_t in_layout, const void* wp, int64_t n, int32_t cin, int32_t cout,
                          int32_t h, int32_t w, void* dz, const void* x1, const void* x2, int32_t c1,
                          const float* chan_bias, const float* gamma, const float* beta, const float* stats,
                          int32_t groups, int32_t act, void* dx1, void* dx2, int32_t dx_layout, const void* add1,
                          const void* add2, const void* add1b, void* ws, int64_t ws_bytes, sp_stream_t stream) {
    if (!dy || !wp || !dz || !x1 || !stats || !dx1 || !ws || (in_layout != 0 && in_layout != 1) ||
        !sp_conv3x3_bf16_gnvjp_supported(n, cin, cout, h, w, c1, groups))
        return SP_EINVAL;
    const int c2 = cout - c1;
    if ((c2 && (!x2 || !dx2)) || (dx_layout != 0 && (dx_layout != 1 || c2)) ||
        ws_bytes < sp_conv3x3_bf16_gnvjp_workspace(n, cout, h, w))
        return SP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t hw = (int64_t)h * w, nc = n * (int64_t)cout;
    const int tiles = static_cast<int>(gnv_tiles(h, w));
    float* part = static_cast<float*>(ws);
    float* co = part + n * tiles * 2 * (int64_t)cout;
    float* co2 = co + 4 * nc;
    const u16* a = static_cast<const u16*>(x1);
    const u16* b = static_cast<const u16*>(x2);
    const u16* d = static_cast<const u16*>(dz);
    gnb_coefs_pass(stats, chan_bias, gamma, beta, n, cout, groups, co, s);
    ConvGn gn{a, b, c1, act ? 1 : 0, co, gamma, part};
    const int ni = static_cast<int>(n);
    if (in_layout)
        conv_bf16_launch<32, false, true, false, true>(static_cast<const u16*>(dy), static_cast<const u16*>(wp), nullptr,
                                                       nullptr, ni, cin, cout, h, w, static_cast<u16*>(dz), s, nullptr,
                                                       1, ConvSc{}, gn);
    else
        conv_bf16_launch<32, false, false, false, true>(static_cast<const u16*>(dy), static_cast<const u16*>(wp),
                                                        nullptr, nullptr, ni, cin, cout, h, w, static_cast<u16*>(dz), s,
                                                        nullptr, 1, ConvSc{}, gn);
    gnb_final_bwd_pass(part, tiles, n, hw, cout, groups, stats, gamma, co, co2, s);
    gnb_bwd_apply_pass(act != 0, false, d, a, b, c1, c2, co, co2, n, hw, static_cast<u16*>(dx1), static_cast<u16*>(dx2),
                       static_cast<const u16*>(add1), static_cast<const u16*>(add2), static_cast<const u16*>(add1b),
                       dx_layout, s);
    return check_launch("sp_conv3x3_bf16_gnvjp");
}

// y = conv3x3(x) + bias (+ res) as sp_conv3x3_bf16_ex, then z = act(GroupNorm(y + chan_bias) gamma + beta)
// as sp_groupnorm_bf16_fwd_ex (z_layout, stats [mean | rstd]) — with the GroupNorm's moments taken in
// the conv's epilogue per 512-pixel tile, shifted by the tile's first pixel (no pass re-reading y).
int sp_conv3x3_bf16_gn_supported(int64_t n, int32_t cin, int32_t cout, int32_t h, int32_t w, int32_t groups) {
    return n > 0 && n <= 65535 && sp_conv3x3_bf16_supported(cin, cout, h, w) && conv_tc(h, w) == 32 &&
           cout % 16 == 0 && sp_groupnorm_bf16_supported(cout, 0, groups) &&
           conv_parts(static_cast<int>(n), cin, cout, h, w) == 1 &&
           n * h * (int64_t)w * std::max(cin, cout) < (int64_t(1) << 40);
}

// workspace bytes (fp32): per-tile moments [n][tiles][3][cout] + coefficients [2][n][cout]
int64_t sp_conv3x3_bf16_gn_workspace(int64_t n, int32_t cout, int32_t h, int32_t w) {
    return 4 * (n * gnv_tiles(h, w) * 3 * (int64_t)cout + 2 * n * (int64_t)cout);
}

int sp_conv3x3_bf16_gn(const void* x, int32_t in_layout, const void* wp, const float* bias, const void* res,
                       int64_t n, int32_t cin, int32_t cout, int32_t h, int32_t w, void* y, const float* chan_bias,
                       const float* gamma, const float* beta, int32_t groups, float eps, int32_t act, void* z,
                       int32_t z_layout, float* stats, void* ws, int64_t ws_bytes, sp_stream_t stream) {
    if (!x || !wp || !y || !z || !stats || !ws || (in_layout != 0 && in_layout != 1) || (z_layout != 0 && z_layout != 1) ||
        !sp_conv3x3_bf16_gn_supported(n, cin, cout, h, w, groups) || ws_bytes < sp_conv3x3_bf16_gn_workspace(n, cout, h, w))
        return SP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t hw = (int64_t)h * w;
    const int tiles = static_cast<int>(gnv_tiles(h, w));
    float* part = static_cast<float*>(ws);
    float* co = part + n * tiles * 3 * (int64_t)cout;
    ConvGn gn{nullptr, nullptr, cout, act ? 1 : 0, chan_bias, gamma, part};
    const int ni = static_cast<int>(n);
    const u16* xx = static_cast<const u16*>(x);
    const u16* ww = static_cast<const u16*>(wp);
    const u16* rr = static_cast<const u16*>(res);
    u16* yy = static_cast<u16*>(y);
    if (in_layout)
        conv_bf16_launch<32, false, true, false, false, true>(xx, ww, bias, rr, ni, cin, cout, h, w, yy, s, nullptr, 1,
                                                              ConvSc{}, gn);
    else
        conv_bf16_launch<32, false, false, false, false, true>(xx, ww, bias, rr, ni, cin, cout, h, w, yy, s, nullptr, 1,
                                                               ConvSc{}, gn);
    gnb_final_fwd_tiles_pass(part, tiles, 512, n, hw, cout, groups, eps, chan_bias, gamma, beta, stats, co, s);
    gnb_apply_pass(act != 0, false, yy, nullptr, cout, 0, co, n, hw, static_cast<u16*>(z), z_layout, s);
    return check_launch("sp_conv3x3_bf16_gn");
}

}  // extern "C"
