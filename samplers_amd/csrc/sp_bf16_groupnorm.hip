// The bf16 priors' GroupNorm (layout rationale: sp_bf16.h):
//
//   k_gnb_stats / _final / _apply / _bwd_*   GroupNorm(+per-(n,c) bias)(+SiLU) forward and
//                        input VJP: per-chunk channel partial sums (shifted), a per-group
//                        finalize in fp64, and a streaming apply — two reads and one write of
//                        the bf16 tensor forward

#define SP_TU 20  // debug-build site numbering (sp_common.h SP_DCHECK)
#include "sp_bf16.h"

#include <type_traits>

namespace sp {

// ---------------------------------------------------------------------------------------------
// GroupNorm over NHWC bf16 (groups of consecutive channels), fp32 statistics.
//
// stats pass (grid: chunks x batch): thread (vector column j, pixel row) accumulates, for its 8
// channels, either the shifted sums  sum (x~ - s_c), sum (x~ - s_c)^2  (x~ = x + chan_bias,
// s_c = x~ at the middle pixel of the chunk, gnb_shift_px: no cancellation when |mean| >> std),
// or for the VJP
// sum g, sum g xhat (g = dy' gamma); the pixel rows of a column meet in LDS in a fixed order and
// one partial per (sample, chunk, channel) is written.  finalize (one wave per (sample, group),
// fp64, fixed order): forward -> mean, rstd and the per-(n, c) affine of the apply
// (y = x sc + sh); VJP -> the per-(n, c) coefficients of dx = A dy' + B x + D.
//
// The shift is per chunk.  The fp32 partials lose (s_c - mean_c)^2 / var_c times their rounding
// (~1e-7) where s_c is an outlier of its channel.  One pixel as the shift of every chunk — the
// sample's first, a corner of the image, as this file had it — put rstd 1e-4 off with 1000 at
// that corner of a 32 x 32 channel; a pixel per chunk costs at most that chunk's partials (the
// error shrinks by the number of chunks), corners are no chunk's middle, and the finalize merges
// the chunks about the group mean in fp64, so shifts that differ between chunks cost nothing.
// ---------------------------------------------------------------------------------------------
constexpr int GNB_TARGET_BLOCKS = 2048;
#ifndef GNB_U
#define GNB_U 4  // pixels whose loads a thread keeps in flight in the streaming GroupNorm loops
#endif

struct GnbGeo {
    int cv, rows, chunks, chunk_px;
};

// non-temporal GroupNorm streams for tensors of at least SP_GNB_NT_MB MB (0 = always, negative =
// never: the default — at 256 MB the microbenchmark's large shapes gain 5-9 % but the PSLD bf16 step
// lost 2 %, profiles/round6/bf16/gn_nt_ab/)
#ifndef SP_GNB_NT_MB
#define SP_GNB_NT_MB -1
#endif
static bool gnb_nt(int64_t n, int c, int64_t hw) {
    return SP_GNB_NT_MB >= 0 && 2 * n * hw * (int64_t)c >= (int64_t)SP_GNB_NT_MB * (1 << 20);
}

static GnbGeo gnb_geo(int64_t n, int c, int64_t hw) {
    GnbGeo g;
    g.cv = c / 8;
    g.rows = g.cv >= kBlock ? 1 : kBlock / g.cv;
    int64_t want = std::max<int64_t>(1, (GNB_TARGET_BLOCKS + n - 1) / n);
    int64_t maxc = std::max<int64_t>(1, hw / (4 * g.rows));
    int64_t ch = std::min<int64_t>(want, maxc);
    ch = std::min<int64_t>(ch, 1024);
    g.chunk_px = static_cast<int>((hw + ch - 1) / ch);
    g.chunks = static_cast<int>((hw + g.chunk_px - 1) / g.chunk_px);
    return g;
}

// GroupNorm streams: NT = non-temporal cache policy on the loads and stores, chosen per call by the
// tensor's size (gnb_nt: an A/B knob, off by default; below the 256 MB last-level cache the second
// pass's re-read hits that cache and NT loses — measured, profiles/round6/bf16/gn_nt_ab/)
template <bool NT>
__device__ __forceinline__ bq_u4 gnb_load(const u16* p) {
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const bq_u4*>(p));
    return *reinterpret_cast<const bq_u4*>(p);
}
#ifndef SP_GNB_NT_STORE
#define SP_GNB_NT_STORE 1  // the NT policy on the stores too (A/B knob)
#endif
template <bool NT>
__device__ __forceinline__ void gnb_store(u16* p, bq_u4 v) {
    if constexpr (NT && SP_GNB_NT_STORE) __builtin_nontemporal_store(v, reinterpret_cast<bq_u4*>(p));
    else *reinterpret_cast<bq_u4*>(p) = v;
}

// one 16-byte vector (8 channels, column j) of pixel p of sample nn, from the part that holds it
template <bool NT = false>
__device__ __forceinline__ bq_u4 gnb_ld(const u16* __restrict__ x1, const u16* __restrict__ x2, int c1, int c2,
                                        int64_t nn, int64_t hw, int64_t p, int j) {
    const int ch = 8 * j;
    if (ch < c1) return gnb_load<NT>(x1 + ((nn * hw + p) * c1 + ch));
    return gnb_load<NT>(x2 + ((nn * hw + p) * c2 + ch - c1));
}

// The pixel whose x~ is the shift of chunk [p0, p1)'s sums: the stats pass and the finalize form it
// identically (gnb_shift).
__device__ __forceinline__ int64_t gnb_shift_px(int64_t p0, int64_t p1) { return p0 + ((p1 - p0) >> 1); }

// MODE 0: forward shifted sums; MODE 1: VJP sums (g, g xhat) given per-(n,c) coefs
// co = [sc | sh | xs | xo] (each n x c fp32) and gamma (c fp32)
template <int MODE, bool ACT, bool NT = false>
__global__ __launch_bounds__(kBlock) void k_gnb_stats(const u16* __restrict__ x1, const u16* __restrict__ x2, int c1,
                                                      int c2, const float* __restrict__ cbias,
                                                      const u16* __restrict__ dz, const float* __restrict__ co,
                                                      const float* __restrict__ gamma, int64_t hw, int chunk_px,
                                                      float* __restrict__ part) {
    __shared__ float red[kBlock * 16];
    const int c = c1 + c2, cv = c / 8, nn = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const int64_t nc = (int64_t)gridDim.y * c;
    const int64_t p0 = (int64_t)chunk * chunk_px, p1 = std::min<int64_t>(hw, p0 + chunk_px);
    for (int jb = 0; jb < cv; jb += kBlock) {  // column blocks (cv > 256 only: 2560 channels)
        const int colw = std::min(cv - jb, kBlock);
        const int rows_here = kBlock / colw;
        const int j = jb + tid % colw, row = tid / colw;
        const bool active = row < rows_here;
        float s1[8] = {}, s2[8] = {};
        if (active) {
            float sh[8] = {}, cbv[8] = {}, k0[8], k1[8], k2[8], k3[8], gm[8];
            if (cbias) {
                const float4 a = *reinterpret_cast<const float4*>(cbias + (int64_t)nn * c + 8 * j);
                const float4 b = *reinterpret_cast<const float4*>(cbias + (int64_t)nn * c + 8 * j + 4);
                cbv[0] = a.x, cbv[1] = a.y, cbv[2] = a.z, cbv[3] = a.w, cbv[4] = b.x, cbv[5] = b.y, cbv[6] = b.z,
                cbv[7] = b.w;
            }
            if constexpr (MODE == 0) {
                float f[8];
                unpack8(gnb_ld(x1, x2, c1, c2, nn, hw, gnb_shift_px(p0, p1), j), f);
#pragma unroll
                for (int e = 0; e < 8; ++e) sh[e] = f[e] + cbv[e];
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int64_t ix = (int64_t)nn * c + 8 * j + e;
                    k0[e] = co[ix], k1[e] = co[nc + ix], k2[e] = co[2 * nc + ix], k3[e] = co[3 * nc + ix];
                    gm[e] = gamma[8 * j + e];
                }
            }
            // one pixel's contribution, from its loaded vectors (x; dz for the VJP)
            auto acc1 = [&](bq_u4 xv, bq_u4 dzv) {
                float f[8];
                unpack8(xv, f);
                if constexpr (MODE == 0) {
                    (void)dzv;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float d = f[e] + cbv[e] - sh[e];
                        s1[e] += d;
                        s2[e] = fmaf(d, d, s2[e]);
                    }
                } else {
                    float dv[8];
                    unpack8(dzv, dv);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float yv = fmaf(f[e], k0[e], k1[e]);
                        float d = dv[e];
                        if constexpr (ACT) {
                            const float sg = __builtin_amdgcn_rcpf(1.f + __expf(-yv));
                            d *= sg * (1.f + yv * (1.f - sg));
                        }
                        const float g = d * gm[e];
                        const float xh = fmaf(f[e], k2[e], k3[e]);
                        s1[e] += g;
                        s2[e] = fmaf(g, xh, s2[e]);
                    }
                }
            };
            auto ldz = [&](int64_t p) {
                if constexpr (MODE == 1) return gnb_load<NT>(dz + ((int64_t)nn * hw + p) * c + 8 * j);
                else return bq_u4{0u, 0u, 0u, 0u};
            };
            // GNB_U pixels' loads in flight per thread, then their sums in pixel order (the same
            // order as one pixel at a time: bit-identical partials)
            int64_t p = p0 + row;
            for (; p + (GNB_U - 1) * rows_here < p1; p += GNB_U * rows_here) {
                bq_u4 xv[GNB_U], dzv[GNB_U];
#pragma unroll
                for (int u = 0; u < GNB_U; ++u) {
                    xv[u] = gnb_ld<NT>(x1, x2, c1, c2, nn, hw, p + u * rows_here, j);
                    dzv[u] = ldz(p + u * rows_here);
                }
#pragma unroll
                for (int u = 0; u < GNB_U; ++u) acc1(xv[u], dzv[u]);
            }
            for (; p < p1; p += rows_here) acc1(gnb_ld(x1, x2, c1, c2, nn, hw, p, j), ldz(p));
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) red[tid * 16 + e] = s1[e], red[tid * 16 + 8 + e] = s2[e];
        __syncthreads();
        // column reduce: thread t < colw sums rows 0 .. rows_here-1 of column t in order
        if (tid < colw) {
            float a1[8] = {}, a2[8] = {};
            for (int rr = 0; rr < rows_here; ++rr) {
                const float* src = red + (rr * colw + tid) * 16;
#pragma unroll
                for (int e = 0; e < 8; ++e) a1[e] += src[e], a2[e] += src[8 + e];
            }
            // partials [n][chunk][2][c]
            float* dst = part + (((int64_t)nn * gridDim.x + chunk) * 2) * c + 8 * (jb + tid);
#pragma unroll
            for (int e = 0; e < 8; ++e) dst[e] = a1[e], dst[c + e] = a2[e];
        }
    }
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// forward finalize: one wave per (n, group).  stats = [mean | rstd] (n*groups each);
// co = [sc | sh] (n*c each): y = x sc + sh.  The group's (chunk, channel) partials are spread
// over the wave's lanes (pair i = lane, lane + 64, ...: channel i % cpg of chunk i / cpg, so a
// row of partials is read by consecutive lanes), each lane sums its pairs in a fixed order in
// fp64, and the wave meets in a fixed butterfly — a handful of loads per lane instead of a
// chain of `chunks` dependent loads on cpg lanes (4 of 64 at 128 channels / 32 groups).
// the shift of channel ch in chunk [p0, p1) of sample nn, as k_gnb_stats MODE 0 forms it
__device__ __forceinline__ float gnb_shift(const u16* __restrict__ x1, const u16* __restrict__ x2, int c1, int c2,
                                           const float* __restrict__ cbias, int64_t nn, int64_t hw, int c, int ch,
                                           int64_t p0, int64_t p1) {
    const float cbv = cbias ? cbias[nn * c + ch] : 0.f;
    const int64_t px = nn * hw + gnb_shift_px(p0, p1);
    return (ch < c1 ? bf1(x1[px * c1 + ch]) : bf1(x2[px * c2 + ch - c1])) + cbv;
}

__global__ __launch_bounds__(64) void k_gnb_final_fwd(const u16* __restrict__ x1, const u16* __restrict__ x2, int c1,
                                                      int c2, const float* __restrict__ cbias,
                                                      const float* __restrict__ part, int chunks, int chunk_px,
                                                      int64_t hw, int groups, float eps,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      float* __restrict__ stats, float* __restrict__ co) {
    const int c = c1 + c2, cpg = c / groups, g = blockIdx.x, nn = blockIdx.y, lane = threadIdx.x;
    const int64_t ng = (int64_t)gridDim.y * groups;
    const int pairs = cpg * chunks;
    const float* __restrict__ pb = part + (int64_t)nn * chunks * 2 * c + g * cpg;  // chunk 0, first channel
    // One pass over the group's (chunk, channel) pairs, in fp64, about a reference r (the first
    // pair's shift): with d = shift - r and P the chunk's pixels, sum (x~ - r) = sum of S1 + P d and
    // sum (x~ - r)^2 = sum of S2 + 2 d S1 + P d^2.  r is one of the group's values, so the
    // cancellation left in var = E2 - E1^2 is (r - mean)^2 / var times 2^-53.
    const double r = gnb_shift(x1, x2, c1, c2, cbias, nn, hw, c, g * cpg, 0, std::min<int64_t>(hw, chunk_px));
    double sa = 0.0, sx = 0.0;
    for (int i = lane; i < pairs; i += 64) {
        const int k = i / cpg, cc = i - k * cpg;
        const float* pp = pb + (int64_t)k * 2 * c + cc;
        const int64_t p0 = (int64_t)k * chunk_px, p1 = std::min<int64_t>(hw, p0 + chunk_px);
        const double d = (double)gnb_shift(x1, x2, c1, c2, cbias, nn, hw, c, g * cpg + cc, p0, p1) - r;
        const double np = (double)(p1 - p0), s1 = pp[0];
        sa += s1 + np * d;
        sx += pp[c] + 2.0 * d * s1 + np * d * d;
    }
    const double cnt = (double)hw * cpg;
    const double m1 = wave_sum_d(sa) / cnt;
    const double mean = r + m1;
    const double var = std::max(0.0, wave_sum_d(sx) / cnt - m1 * m1);
    const float rstd = (float)(1.0 / sqrt(var + (double)eps));
    const float meanf = (float)mean;
    if (lane == 0) stats[(int64_t)nn * groups + g] = meanf, stats[ng + (int64_t)nn * groups + g] = rstd;
    const int64_t nc = (int64_t)gridDim.y * c;
    for (int cc = lane; cc < cpg; cc += 64) {
        const int ch = g * cpg + cc;
        const float cbv = cbias ? cbias[(int64_t)nn * c + ch] : 0.f;
        const float sc = rstd * (gamma ? gamma[ch] : 1.f);
        co[(int64_t)nn * c + ch] = sc;
        co[nc + (int64_t)nn * c + ch] = (beta ? beta[ch] : 0.f) + (cbv - meanf) * sc;
    }
}

// forward finalize from per-tile shifted moments (the FS conv epilogue): part [n][tile][3][c] =
// sum(d), sum(d^2), K (d = x~ - K over the tile's P pixels); per group in fp64: the mean from
// sum(d) + P K, then sum (x~ - mean)^2 = sum over (tile, channel) of S2 + 2 (K - mean) S1 + P (K - mean)^2.
// Outputs as k_gnb_final_fwd.
__global__ __launch_bounds__(64) void k_gnb_final_fwd_tiles(const float* __restrict__ part, int tiles, int64_t px,
                                                            int64_t hw, int c, int groups, float eps,
                                                            const float* __restrict__ cbias,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ stats,
                                                            float* __restrict__ co) {
    const int cpg = c / groups, g = blockIdx.x, nn = blockIdx.y, lane = threadIdx.x;
    const int64_t ng = (int64_t)gridDim.y * groups;
    const int pairs = cpg * tiles;
    const float* __restrict__ pb = part + (int64_t)nn * tiles * 3 * c + g * cpg;
    double sa = 0.0;
    for (int i = lane; i < pairs; i += 64) {
        const int k = i / cpg, cc = i - k * cpg;
        const float* pp = pb + (int64_t)k * 3 * c + cc;
        sa += (double)pp[0] + (double)px * pp[2 * c];
    }
    const double cnt = (double)hw * cpg;
    const double mean = wave_sum_d(sa) / cnt;
    double sx = 0.0;
    for (int i = lane; i < pairs; i += 64) {
        const int k = i / cpg, cc = i - k * cpg;
        const float* pp = pb + (int64_t)k * 3 * c + cc;
        const double dm = (double)pp[2 * c] - mean;
        sx += (double)pp[c] + 2.0 * dm * pp[0] + (double)px * dm * dm;
    }
    const double var = std::max(0.0, wave_sum_d(sx) / cnt);
    const float rstd = (float)(1.0 / sqrt(var + (double)eps));
    const float meanf = (float)mean;
    if (lane == 0) stats[(int64_t)nn * groups + g] = meanf, stats[ng + (int64_t)nn * groups + g] = rstd;
    const int64_t nc = (int64_t)gridDim.y * c;
    for (int cc = lane; cc < cpg; cc += 64) {
        const int ch = g * cpg + cc;
        const float cbv = cbias ? cbias[(int64_t)nn * c + ch] : 0.f;
        const float sc = rstd * (gamma ? gamma[ch] : 1.f);
        co[(int64_t)nn * c + ch] = sc;
        co[nc + (int64_t)nn * c + ch] = (beta ? beta[ch] : 0.f) + (cbv - meanf) * sc;
    }
}

// per-(n, c) coefficients for the VJP from the forward's stats: co = [sc | sh | xs | xo]
// (y = x sc + sh, xhat = x xs + xo)
__global__ void k_gnb_coefs(const float* __restrict__ stats, const float* __restrict__ cbias,
                            const float* __restrict__ gamma, const float* __restrict__ beta, int n, int c,
                            int groups, float* __restrict__ co) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nc = (int64_t)n * c;
    if (i >= nc) return;
    const int nn = static_cast<int>(i / c), ch = static_cast<int>(i - (int64_t)nn * c), g = ch / (c / groups);
    const float mean = stats[(int64_t)nn * groups + g], rstd = stats[(int64_t)n * groups + (int64_t)nn * groups + g];
    const float cbv = cbias ? cbias[i] : 0.f;
    const float sc = rstd * (gamma ? gamma[ch] : 1.f);
    co[i] = sc;
    co[nc + i] = (beta ? beta[ch] : 0.f) + (cbv - mean) * sc;
    co[2 * nc + i] = rstd;
    co[3 * nc + i] = (cbv - mean) * rstd;
}

// VJP finalize: one wave per (n, group): m1 = mean(g), m2 = mean(g xhat) over the group ->
// dx = A dy' + B x + D with A = rstd gamma_c, B = -rstd^2 m2, D = -rstd (m1 + m2 xo_c);
// co2 = [A | B | D]
__global__ __launch_bounds__(64) void k_gnb_final_bwd(const float* __restrict__ part, int chunks, int64_t hw, int c,
                                                      int groups, const float* __restrict__ stats,
                                                      const float* __restrict__ gamma, const float* __restrict__ co,
                                                      float* __restrict__ co2) {
    const int cpg = c / groups, g = blockIdx.x, nn = blockIdx.y, lane = threadIdx.x, n = gridDim.y;
    const int pairs = cpg * chunks;
    const float* __restrict__ pb = part + (int64_t)nn * chunks * 2 * c + g * cpg;
    double s1 = 0.0, s2 = 0.0;  // (chunk, channel) pairs spread over the lanes as k_gnb_final_fwd
    for (int i = lane; i < pairs; i += 64) {
        const int k = i / cpg, cc = i - k * cpg;
        const float* pp = pb + (int64_t)k * 2 * c + cc;
        s1 += pp[0];
        s2 += pp[c];
    }
    const double cnt = (double)hw * cpg;
    const float m1 = (float)(wave_sum_d(s1) / cnt), m2 = (float)(wave_sum_d(s2) / cnt);
    const float rstd = stats[(int64_t)n * groups + (int64_t)nn * groups + g];
    const int64_t nc = (int64_t)n * c;
    for (int cc = lane; cc < cpg; cc += 64) {
        const int ch = g * cpg + cc;
        const int64_t i = (int64_t)nn * c + ch;
        co2[i] = rstd * (gamma ? gamma[ch] : 1.f);
        co2[nc + i] = -rstd * rstd * m2;
        co2[2 * nc + i] = -rstd * (m1 + m2 * co[3 * nc + i]);
    }
}

// forward apply: z = act(x sc + sh) over the concatenated channels.  Grid (chunks, batch) as the
// stats pass: a thread owns one 8-channel column of the sample, keeps its (n, c) coefficients in
// registers and walks the chunk's pixels (the block reads rows of C channels contiguously).
template <bool ACT, bool NT = false>
__global__ __launch_bounds__(kBlock) void k_gnb_apply(const u16* __restrict__ x1, const u16* __restrict__ x2, int c1,
                                                      int c2, const float* __restrict__ co, int64_t hw, int chunk_px,
                                                      u16* __restrict__ z, int blk) {
    const int c = c1 + c2, cv = c / 8, nn = blockIdx.y, tid = threadIdx.x;
    const int64_t nc = (int64_t)gridDim.y * c;
    const int64_t p0 = (int64_t)blockIdx.x * chunk_px, p1 = std::min<int64_t>(hw, p0 + chunk_px);
    for (int jb = 0; jb < cv; jb += kBlock) {
        const int colw = std::min(cv - jb, kBlock), rows = kBlock / colw;
        const int j = jb + tid % colw, row = tid / colw;
        if (row >= rows) continue;
        const float* sc = co + (int64_t)nn * c + 8 * j;
        const float* sh = co + nc + (int64_t)nn * c + 8 * j;
        const float4 a0 = *reinterpret_cast<const float4*>(sc), a1 = *reinterpret_cast<const float4*>(sc + 4);
        const float4 b0 = *reinterpret_cast<const float4*>(sh), b1 = *reinterpret_cast<const float4*>(sh + 4);
        const float sa[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const float sb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
        auto one = [&](bq_u4 xv, int64_t p) {
            float f[8];
            unpack8(xv, f);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float yv = fmaf(f[e], sa[e], sb[e]);
                f[e] = ACT ? silu_f(yv) : yv;
            }
            // blk: z in the channel-blocked layout [n][c / 16][hw][16] the conv tile reads best
            const int64_t zo = blk ? (((int64_t)nn * (c >> 4) + (j >> 1)) * hw + p) * 16 + 8 * (j & 1)
                                   : ((int64_t)nn * hw + p) * c + 8 * j;
            gnb_store<NT>(z + zo, pack8(f));
        };
        int64_t p = p0 + row;
        for (; p + (GNB_U - 1) * rows < p1; p += GNB_U * rows) {  // GNB_U pixels' loads in flight
            bq_u4 xv[GNB_U];
#pragma unroll
            for (int u = 0; u < GNB_U; ++u) xv[u] = gnb_ld<NT>(x1, x2, c1, c2, nn, hw, p + u * rows, j);
#pragma unroll
            for (int u = 0; u < GNB_U; ++u) one(xv[u], p + u * rows);
        }
        for (; p < p1; p += rows) one(gnb_ld(x1, x2, c1, c2, nn, hw, p, j), p);
    }
}

// VJP apply: dx = A dy' + B x + D (+ add1 / add2 / add1b), written to the parts' layouts; grid
// and column ownership as k_gnb_apply (the five (n, c) coefficient rows held in registers)
template <bool ACT, bool NT = false>
__global__ __launch_bounds__(kBlock) void k_gnb_bwd_apply(const u16* __restrict__ dz, const u16* __restrict__ x1,
                                                          const u16* __restrict__ x2, int c1, int c2,
                                                          const float* __restrict__ co, const float* __restrict__ co2,
                                                          int64_t hw, int chunk_px, u16* __restrict__ dx1,
                                                          u16* __restrict__ dx2, const u16* __restrict__ add1,
                                                          const u16* __restrict__ add2,
                                                          const u16* __restrict__ add1b, int blk) {
    const int c = c1 + c2, cv = c / 8, nn = blockIdx.y, tid = threadIdx.x;
    const int64_t nc = (int64_t)gridDim.y * c;
    const int64_t p0 = (int64_t)blockIdx.x * chunk_px, p1 = std::min<int64_t>(hw, p0 + chunk_px);
    for (int jb = 0; jb < cv; jb += kBlock) {
        const int colw = std::min(cv - jb, kBlock), rows = kBlock / colw;
        const int j = jb + tid % colw, row = tid / colw;
        if (row >= rows) continue;
        const int64_t ci = (int64_t)nn * c + 8 * j;
        float ka[8], kb[8], kd[8], ksc[8], ksh[8];
        ld8f(co2 + ci, ka);
        ld8f(co2 + nc + ci, kb);
        ld8f(co2 + 2 * nc + ci, kd);
        if constexpr (ACT) {
            ld8f(co + ci, ksc);
            ld8f(co + nc + ci, ksh);
        }
        const int ch = 8 * j;
        const bool first = ch < c1;
        const int cp = first ? c1 : c2, chp = first ? ch : ch - c1;
        u16* __restrict__ dst = first ? dx1 : dx2;
        // blk & 2: add1 is one addend over the concatenated channels ([n][hw][c1 + c2], e.g. the
        // 1x1 shortcut's input gradient from one GEMM), add2 unused
        const bool acat = (blk & 2) != 0;
        const u16* __restrict__ a = acat ? add1 : first ? add1 : add2;
        const u16* __restrict__ ab = first ? add1b : nullptr;
        const u16* __restrict__ xs = first ? x1 : x2;
        // one pixel from its loaded vectors (x, dy', and the addends or zeros)
        auto one = [&](bq_u4 xv, bq_u4 dv, bq_u4 av, bq_u4 bv, int64_t off, int64_t p) {
            float f[8], d[8], o[8];
            unpack8(xv, f);
            unpack8(dv, d);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float dd = d[e];
                if constexpr (ACT) {
                    const float yv = fmaf(f[e], ksc[e], ksh[e]);
                    const float sg = __builtin_amdgcn_rcpf(1.f + __expf(-yv));
                    dd *= sg * (1.f + yv * (1.f - sg));
                }
                o[e] = fmaf(ka[e], dd, fmaf(kb[e], f[e], kd[e]));
            }
            if (a) {
                float t[8];
                unpack8(av, t);
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] += t[e];
            }
            if (ab) {
                float t[8];
                unpack8(bv, t);
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] += t[e];
            }
            // blk & 1 (one part): dx in the channel-blocked layout [n][c / 16][hw][16]
            const int64_t oo = (blk & 1) ? (((int64_t)nn * (cp >> 4) + (chp >> 4)) * hw + p) * 16 + (chp & 15) : off;
            gnb_store<NT>(dst + oo, pack8(o));
        };
        const bq_u4 zero4 = {0u, 0u, 0u, 0u};
        auto ld = [&](const u16* __restrict__ src, int64_t off) {
            return src ? gnb_load<NT>(src + off) : zero4;
        };
        int64_t p = p0 + row;
        for (; p + (GNB_U - 1) * rows < p1; p += GNB_U * rows) {  // GNB_U pixels' loads in flight
            bq_u4 xv[GNB_U], dv[GNB_U], av[GNB_U], bv[GNB_U];
#pragma unroll
            for (int u = 0; u < GNB_U; ++u) {
                const int64_t pp = p + u * rows, off = ((int64_t)nn * hw + pp) * cp + chp;
                xv[u] = gnb_load<NT>(xs + off);
                dv[u] = gnb_load<NT>(dz + ((int64_t)nn * hw + pp) * c + ch);
                av[u] = ld(a, acat ? ((int64_t)nn * hw + pp) * c + ch : off);
                bv[u] = ld(ab, off);
            }
#pragma unroll
            for (int u = 0; u < GNB_U; ++u)
                one(xv[u], dv[u], av[u], bv[u], ((int64_t)nn * hw + p + u * rows) * cp + chp, p + u * rows);
        }
        for (; p < p1; p += rows) {
            const int64_t off = ((int64_t)nn * hw + p) * cp + chp;
            one(*reinterpret_cast<const bq_u4*>(xs + off), *reinterpret_cast<const bq_u4*>(dz + ((int64_t)nn * hw + p) * c + ch),
                ld(a, acat ? ((int64_t)nn * hw + p) * c + ch : off), ld(ab, off), off, p);
        }
    }
}

// The passes as host calls (declared in sp_bf16.h): one launch each, the ACT / NT dispatch inside.
static dim3 final_grid(int groups, int64_t n) { return dim3(groups, static_cast<unsigned>(n)); }

// f(bool_constant ACT, bool_constant NT) for the runtime (act, nt)
template <typename F>
static void gnb_act_nt(bool act, bool nt, F&& f) {
    if (act) nt ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
    else nt ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}

void gnb_coefs_pass(const float* stats, const float* cbias, const float* gamma, const float* beta, int64_t n, int c,
                    int groups, float* co, hipStream_t s) {
    launch(0, k_gnb_coefs, dim3(static_cast<unsigned>((n * c + kBlock - 1) / kBlock)), dim3(kBlock), s, stats, cbias,
           gamma, beta, static_cast<int>(n), c, groups, co);
}

void gnb_stats_pass(int mode, bool act, bool nt, const u16* x1, const u16* x2, int c1, int c2, const float* cbias,
                    const u16* dz, const float* co, const float* gamma, int64_t n, int64_t hw, float* part,
                    hipStream_t s) {
    const GnbGeo g = gnb_geo(n, c1 + c2, hw);
    auto pass = [&](auto kern) {
        launch(0, kern, dim3(g.chunks, static_cast<unsigned>(n)), dim3(kBlock), s, x1, x2, c1, c2, cbias, dz, co, gamma,
               hw, g.chunk_px, part);
    };
    if (mode == 0) nt ? pass(k_gnb_stats<0, false, true>) : pass(k_gnb_stats<0, false, false>);
    else gnb_act_nt(act, nt, [&](auto a, auto t) { pass(k_gnb_stats<1, decltype(a)::value, decltype(t)::value>); });
}

void gnb_final_fwd_pass(const u16* x1, const u16* x2, int c1, int c2, const float* cbias, const float* part, int chunks,
                        int64_t n, int64_t hw, int groups, float eps, const float* gamma, const float* beta,
                        float* stats, float* co, hipStream_t s) {
    const GnbGeo g = gnb_geo(n, c1 + c2, hw);  // the stats pass's chunking (chunks == g.chunks)
    launch(0, k_gnb_final_fwd, final_grid(groups, n), dim3(64), s, x1, x2, c1, c2, cbias, part, chunks, g.chunk_px, hw,
           groups, eps, gamma, beta, stats, co);
}

void gnb_final_fwd_tiles_pass(const float* part, int tiles, int64_t px, int64_t n, int64_t hw, int c, int groups,
                              float eps, const float* cbias, const float* gamma, const float* beta, float* stats,
                              float* co, hipStream_t s) {
    launch(0, k_gnb_final_fwd_tiles, final_grid(groups, n), dim3(64), s, part, tiles, px, hw, c, groups, eps, cbias,
           gamma, beta, stats, co);
}

void gnb_final_bwd_pass(const float* part, int chunks, int64_t n, int64_t hw, int c, int groups, const float* stats,
                        const float* gamma, const float* co, float* co2, hipStream_t s) {
    launch(0, k_gnb_final_bwd, final_grid(groups, n), dim3(64), s, part, chunks, hw, c, groups, stats, gamma, co, co2);
}

void gnb_apply_pass(bool act, bool nt, const u16* x1, const u16* x2, int c1, int c2, const float* co, int64_t n,
                    int64_t hw, u16* z, int z_layout, hipStream_t s) {
    const GnbGeo g = gnb_geo(n, c1 + c2, hw);
    gnb_act_nt(act, nt, [&](auto a, auto t) {
        launch(0, k_gnb_apply<decltype(a)::value, decltype(t)::value>, dim3(g.chunks, static_cast<unsigned>(n)),
               dim3(kBlock), s, x1, x2, c1, c2, co, hw, g.chunk_px, z, z_layout);
    });
}

void gnb_bwd_apply_pass(bool act, bool nt, const u16* dz, const u16* x1, const u16* x2, int c1, int c2,
                        const float* co, const float* co2, int64_t n, int64_t hw, u16* dx1, u16* dx2,
                        const u16* add1, const u16* add2, const u16* add1b, int dx_layout, hipStream_t s) {
    const GnbGeo g = gnb_geo(n, c1 + c2, hw);
    gnb_act_nt(act, nt, [&](auto a, auto t) {
        launch(0, k_gnb_bwd_apply<decltype(a)::value, decltype(t)::value>, dim3(g.chunks, static_cast<unsigned>(n)),
               dim3(kBlock), s, dz, x1, x2, c1, c2, co, co2, hw, g.chunk_px, dx1, dx2, add1, add2, add1b, dx_layout);
    });
}

}  // namespace sp

using namespace sp;

extern "C" {

// ---- GroupNorm ------------------------------------------------------------------------------

int sp_groupnorm_bf16_supported(int32_t c1, int32_t c2, int32_t groups) {
    const int c = c1 + c2;
    return c1 > 0 && c1 % 8 == 0 && c2 >= 0 && c2 % 8 == 0 && groups > 0 && c % groups == 0 && c <= 8 * 1024;
}

// workspace bytes (fp32): partials [n][chunks][2][c] + coefficients [4][n][c] + [3][n][c]
int64_t sp_groupnorm_bf16_workspace(int64_t n, int32_t c, int64_t hw) {
    const GnbGeo g = gnb_geo(n, c, hw);
    return 4 * (n * g.chunks * 2 * (int64_t)c + 7 * n * (int64_t)c);
}

// z[n][hw][c] = act(GroupNorm(cat(x1, x2) + chan_bias[n][c]) * gamma + beta), NHWC bf16;
// stats = [mean | rstd] (2 n groups fp32, for the VJP); gamma / beta / chan_bias fp32 or NULL.
int sp_groupnorm_bf16_fwd(const void* x1, const void* x2, int32_t c1, int32_t c2, const float* chan_bias,
                          const float* gamma, const float* beta, int64_t n, int64_t hw, int32_t groups, float eps,
                          int32_t act, void* z, float* stats, void* ws, int64_t ws_bytes, sp_stream_t stream) {
    return sp_groupnorm_bf16_fwd_ex(x1, x2, c1, c2, chan_bias, gamma, beta, n, hw, groups, eps, act, z, 0, stats, ws,
                                    ws_bytes, stream);
}

// z_layout 1: z in the channel-blocked layout [n][c / 16][hw][16] (c % 16 == 0), the conv tile's
// preferred input (sp_conv3x3_bf16_ex)
int sp_groupnorm_bf16_fwd_ex(const void* x1, const void* x2, int32_t c1, int32_t c2, const float* chan_bias,
                             const float* gamma, const float* beta, int64_t n, int64_t hw, int32_t groups, float eps,
                             int32_t act, void* z, int32_t z_layout, float* stats, void* ws, int64_t ws_bytes,
                             sp_stream_t stream) {
    if (!x1 || (c2 && !x2) || !z || !stats || !ws || n <= 0 || hw <= 0 || !sp_groupnorm_bf16_supported(c1, c2, groups))
        return SP_EINVAL;
    if (z_layout != 0 && (z_layout != 1 || (c1 + c2) % 16)) return SP_EINVAL;
    const int c = c1 + c2;
    if (ws_bytes < sp_groupnorm_bf16_workspace(n, c, hw) || n * hw * c >= (int64_t(1) << 40) || n > 65535)
        return SP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const GnbGeo g = gnb_geo(n, c, hw);
    float* part = static_cast<float*>(ws);
    float* co = part + n * g.chunks * 2 * (int64_t)c;
    const u16* a = static_cast<const u16*>(x1);
    const u16* b = static_cast<const u16*>(x2);
    const bool nt = gnb_nt(n, c, hw);
    gnb_stats_pass(0, false, nt, a, b, c1, c2, chan_bias, nullptr, nullptr, nullptr, n, hw, part, s);
    gnb_final_fwd_pass(a, b, c1, c2, chan_bias, part, g.chunks, n, hw, groups, eps, gamma, beta, stats, co, s);
    gnb_apply_pass(act != 0, nt, a, b, c1, c2, co, n, hw, static_cast<u16*>(z), z_layout, s);
    return check_launch("sp_groupnorm_bf16_fwd");
}

// input VJP of sp_groupnorm_bf16_fwd given its stats: dx1 / dx2 (the parts' layouts) =
// GN^T dz (+ add1 / add2, + add1b into dx1); the outputs may alias the addends.
int sp_groupnorm_bf16_bwd(const void* dz, const void* x1, const void* x2, int32_t c1, int32_t c2,
                          const float* chan_bias, const float* gamma, const float* beta, const float* stats,
                          int64_t n, int64_t hw, int32_t groups, int32_t act, void* dx1, void* dx2, const void* add1,
                          const void* add2, const void* add1b, void* ws, int64_t ws_bytes, sp_stream_t stream) {
    return sp_groupnorm_bf16_bwd_ex(dz, x1, x2, c1, c2, chan_bias, gamma, beta, stats, n, hw, groups, act, dx1, dx2,
                                    0, add1, add2, add1b, ws, ws_bytes, stream);
}

// dx_layout 1 (one part, c2 == 0, c1 % 16 == 0): dx1 in the channel-blocked layout [n][c / 16][hw][16]
// (the addends stay NHWC); dx_layout 2: dx1 / dx2 NHWC and add1 one addend over the concatenated
// channels [n][hw][c1 + c2] (add2 NULL; the outputs must not alias it)
int sp_groupnorm_bf16_bwd_ex(const void* dz, const void* x1, const void* x2, int32_t c1, int32_t c2,
                             const float* chan_bias, const float* gamma, const float* beta, const float* stats,
                             int64_t n, int64_t hw, int32_t groups, int32_t act, void* dx1, void* dx2, int32_t dx_layout,
                             const void* add1, const void* add2, const void* add1b, void* ws, int64_t ws_bytes,
                             sp_stream_t stream) {
    if (!dz || !x1 || (c2 && (!x2 || !dx2)) || !dx1 || !stats || !ws || n <= 0 || hw <= 0 ||
        !sp_groupnorm_bf16_supported(c1, c2, groups))
        return SP_EINVAL;
    if (dx_layout != 0 && (dx_layout != 1 || c2 || c1 % 16) && (dx_layout != 2 || add2)) return SP_EINVAL;
    const int c = c1 + c2;
    if (ws_bytes < sp_groupnorm_bf16_workspace(n, c, hw) || n * hw * c >= (int64_t(1) << 40) || n > 65535)
        return SP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const GnbGeo g = gnb_geo(n, c, hw);
    float* part = static_cast<float*>(ws);
    float* co = part + n * g.chunks * 2 * (int64_t)c;
    float* co2 = co + 4 * n * (int64_t)c;
    const u16* a = static_cast<const u16*>(x1);
    const u16* b = static_cast<const u16*>(x2);
    const u16* d = static_cast<const u16*>(dz);
    const bool nt = gnb_nt(n, c, hw);
    gnb_coefs_pass(stats, chan_bias, gamma, beta, n, c, groups, co, s);
    gnb_stats_pass(1, act != 0, nt, a, b, c1, c2, chan_bias, d, co, gamma, n, hw, part, s);
    gnb_final_bwd_pass(part, g.chunks, n, hw, c, groups, stats, gamma, co, co2, s);
    gnb_bwd_apply_pass(act != 0, nt, d, a, b, c1, c2, co, co2, n, hw, static_cast<u16*>(dx1), static_cast<u16*>(dx2),
                       static_cast<const u16*>(add1), static_cast<const u16*>(add2), static_cast<const u16*>(add1b),
                       dx_layout, s);
    return check_launch("sp_groupnorm_bf16_bwd");
}

}  // extern "C"
