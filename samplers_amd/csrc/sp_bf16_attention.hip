// The bf16 priors' attention (the MFMA's C layout and fragments: sp_bf16.h):
//
//   k_attnb_fwd<D>       multi-head attention softmax(q k^T / sqrt(d)) v on bf16 q / k / v
//                        (self or cross, keys past m masked), output bf16, row log-sum-exp fp32
//   k_attnb_delta / _dq / _dkv<D>   its VJP (FlashAttention-2 recurrence)

#define SP_TU 22  // debug-build site numbering (sp_common.h SP_DCHECK)
#include "sp_bf16.h"

namespace sp {

// ---------------------------------------------------------------------------------------------
// Multi-head attention on bf16 q / k / v (the SD 1.5 UNet's attn1 / attn2 at the reference's
// bf16): the structure of k_attn6_fwd (sp_attention6.hip) with one bf16 term per operand.
// Per wave 32 queries; per 32-key block S^T = K Q^T (K rows from LDS as A, Q^T in registers as
// B, d padded to 16), the softmax on the lane-local query column (scores scaled by
// scale log2 e in fp32), O^T += V^T P^T with P^T packed to bf16 straight from the S^T
// accumulators (key order inside the MFMA's K = the C layout's, V^T staged in that order).
// Keys past m are masked (-inf); queries past n are computed on zero rows and not stored.
// ---------------------------------------------------------------------------------------------
constexpr float AB_LOG2E = 1.4426950408889634f;
constexpr float AB_LN2 = 0.6931471805599453f;
constexpr int AB_QW = 32, AB_WB = 4 * AB_QW;
constexpr float AB_LAZY = 8.f;


template <int D>
struct AbGeo {
    static_assert(D % 8 == 0 && D <= 160, "head dim");
    static constexpr int DK = (D + 15) / 16;
    static constexpr int DKP = DK * 16;
    static constexpr int DT = (D + 31) / 32;
    static constexpr int SB = 64;
    static constexpr int KROW = DKP + 8;   // bf16 per K row in LDS
    static constexpr int IMG = SB * KROW + 32 * DT;  // a natural image + the columns a last-row tr read reaches
    static constexpr int NVU = (SB / 2 * (D / 8) + kBlock - 1) / kBlock;      // V (2 keys x 8 d) units
};

// a stage of SB rows (row pairs 2p, 2p + 1 x 8 d per unit) into registers.  Rows >= limit read
// row limit - 1 instead (unconditional loads: a select on a loaded value, or a zero written into
// a load's destination, makes the compiler wait for the whole stage's loads at once); the
// kernels give such rows no weight (keys past m: P = 0; queries past n: lse = +inf, delta = 0)
template <int D>
__device__ __forceinline__ void ab_ld_pairs(const u16* __restrict__ src, int64_t rs, int base, int limit,
                                            bq_u4 (&st)[AbGeo<D>::NVU][2]) {
    using G = AbGeo<D>;
#pragma unroll
    for (int j = 0; j < G::NVU; ++j) {
        const int u = threadIdx.x + j * kBlock;
        if (u < G::SB / 2 * (D / 8)) {
            const int p = u / (D / 8), d0 = 8 * (u - p * (D / 8));
            const int r0 = min(base + 2 * p, limit - 1), r1 = min(base + 2 * p + 1, limit - 1);
            st[j][0] = *reinterpret_cast<const bq_u4*>(src + (int64_t)r0 * rs + d0);
            st[j][1] = *reinterpret_cast<const bq_u4*>(src + (int64_t)r1 * rs + d0);
        }
    }
}

// natural image [SB][KROW]
template <int D>
__device__ __forceinline__ void ab_st_nat(u16* img, const bq_u4 (&st)[AbGeo<D>::NVU][2]) {
    using G = AbGeo<D>;
#pragma unroll
    for (int j = 0; j < G::NVU; ++j) {
        const int u = threadIdx.x + j * kBlock;
        if (u < G::SB / 2 * (D / 8)) {
            const int p = u / (D / 8), d0 = 8 * (u - p * (D / 8));
            *reinterpret_cast<bq_u4*>(img + (2 * p) * G::KROW + d0) = st[j][0];
            *reinterpret_cast<bq_u4*>(img + (2 * p + 1) * G::KROW + d0) = st[j][1];
        }
    }
}

typedef short ab_s4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) ab_s4 ab_lds_s4;

// The A fragment of a transposed operand (rows d = 32 dt .. +31, K = 16 rows of a natural
// [rows][KROW] image in the C layout's order: element j of lane half h is row
// row0 + 8 (j >> 2) + 4 h + (j & 3)) read straight from the natural image with two
// ds_read_b64_tr_b16 (T10: lane 4q + p of a 16-lane group gives the address of row q, columns
// 4p .. 4p + 3, and receives column `lane % 16` of the 4 rows) — no transposed copy in LDS.
// trb = img + (4 h + q) KROW + 16 g + 4 p for lane (h, g, q, p); off = row0 KROW + 32 dt.
template <int KROW>
__device__ __forceinline__ bq_u4 ab_tr(const u16* trb, int off) {
    const ab_s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ab_lds_s4*)(trb + off));
    const ab_s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ab_lds_s4*)(trb + off + 8 * KROW));
    return bq_u4{__builtin_bit_cast(bq_u2, lo)[0], __builtin_bit_cast(bq_u2, lo)[1], __builtin_bit_cast(bq_u2, hi)[0],
                 __builtin_bit_cast(bq_u2, hi)[1]};
}

__device__ __forceinline__ int ab_trlane(int lane, int krow) {
    return (4 * (lane >> 5) + ((lane >> 2) & 3)) * krow + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
}

template <int D>
__global__ __launch_bounds__(kBlock) void k_attnb_fwd(const u16* __restrict__ q, const u16* __restrict__ k,
                                                      const u16* __restrict__ v, int n, int m, int heads,
                                                      int rsq, int rskv, int kv_shared, int ro, float sl2,
                                                      u16* __restrict__ out, float* __restrict__ lse) {
    using G = AbGeo<D>;
    __shared__ __attribute__((aligned(16))) u16 Ks[G::IMG];
    __shared__ __attribute__((aligned(16))) u16 Vs[G::IMG];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int bh = blockIdx.y, b = bh / heads, hd = bh - b * heads;
    const int q0 = blockIdx.x * AB_WB + wv * AB_QW;
    const u16* __restrict__ qb = q + (int64_t)b * n * rsq + hd * D;
    const int64_t kvb = (kv_shared ? 0 : (int64_t)b * m * rskv) + hd * D;

    if constexpr (G::DKP > D) {  // K's padding columns: zero once
        for (int i = tid; i < G::SB; i += kBlock)
#pragma unroll
            for (int cc = D; cc < G::DKP; cc += 2) *reinterpret_cast<unsigned*>(Ks + i * G::KROW + cc) = 0u;
    }
    // Q^T as B: lane (query r, half hh) holds Q[q0 + r][16 s + 8 hh + j]
    bq_u4 qf[G::DK];
    const int qq = q0 + r;
#pragma unroll
    for (int s = 0; s < G::DK; ++s) {
        const int d0 = 16 * s + 8 * hh;
        qf[s] = (d0 + 8 <= D && qq < n) ? *reinterpret_cast<const bq_u4*>(qb + (int64_t)qq * rsq + d0)
                                        : bq_u4{0u, 0u, 0u, 0u};
    }
    bq_f16 o[G::DT];
#pragma unroll
    for (int dt = 0; dt < G::DT; ++dt) o[dt] = bq_f16{};
    float mx = -INFINITY, l = 0.f;

    const int nst = (m + G::SB - 1) / G::SB;
    bq_u4 ks[G::NVU][2], vs[G::NVU][2];
    const u16* trb = Vs + ab_trlane(lane, G::KROW);
    ab_ld_pairs<D>(k + kvb, rskv, 0, m, ks);
    ab_ld_pairs<D>(v + kvb, rskv, 0, m, vs);
    for (int si = 0; si < nst; ++si) {
        __syncthreads();
        ab_st_nat<D>(Ks, ks);
        ab_st_nat<D>(Vs, vs);
        __syncthreads();
        if (si + 1 < nst) {
            ab_ld_pairs<D>(k + kvb, rskv, (si + 1) * G::SB, m, ks);
            ab_ld_pairs<D>(v + kvb, rskv, (si + 1) * G::SB, m, vs);
        }
        const int kbase = si * G::SB;
#pragma unroll
        for (int kb32 = 0; kb32 < G::SB / 32; ++kb32) {
            if (kbase + kb32 * 32 >= m) break;  // wave-uniform
            bq_f16 sv = bq_f16{};
#pragma unroll
            for (int s = 0; s < G::DK; ++s) {
                const bq_u4 kf = *reinterpret_cast<const bq_u4*>(Ks + (kb32 * 32 + r) * G::KROW + 16 * s + 8 * hh);
                sv = bq_mfma(kf, qf[s], sv);
            }
            float bm = -INFINITY;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = kbase + kb32 * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh;
                sv[i] = key < m ? sv[i] * sl2 : -INFINITY;
                bm = fmaxf(bm, sv[i]);
            }
            bm = fmaxf(bm, __shfl_xor(bm, 32));
            const float mn = bm > mx + AB_LAZY ? bm : mx;
            const float corr = __builtin_amdgcn_exp2f(mx - mn);
            mx = mn;
            float p[16], ps = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                p[i] = __builtin_amdgcn_exp2f(sv[i] - mn);
                ps += p[i];
            }
            l = fmaf(l, corr, ps);
            if (__builtin_amdgcn_ballot_w64(corr != 1.f))
#pragma unroll
                for (int dt = 0; dt < G::DT; ++dt) o[dt] *= corr;
            bq_u4 pf[2];
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
                pf[kk] = bq_u4{pk2(p[8 * kk], p[8 * kk + 1]), pk2(p[8 * kk + 2], p[8 * kk + 3]),
                               pk2(p[8 * kk + 4], p[8 * kk + 5]), pk2(p[8 * kk + 6], p[8 * kk + 7])};
#pragma unroll
            for (int dt = 0; dt < G::DT; ++dt)
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    const bq_u4 vf = ab_tr<G::KROW>(trb, (kb32 * 32 + kk * 16) * G::KROW + 32 * dt);
                    o[dt] = bq_mfma(vf, pf[kk], o[dt]);
                }
        }
    }
    const float tot = l + __shfl_xor(l, 32);
    const float inv = 1.f / tot;
    if (qq >= n) return;
    u16* orow = out + (int64_t)b * n * ro + hd * D + (int64_t)qq * ro;
#pragma unroll
    for (int dt = 0; dt < G::DT; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int d0 = 32 * dt + 8 * g4 + 4 * hh;
            if (d0 + 4 <= D)
                *reinterpret_cast<bq_u2*>(orow + d0) = bq_u2{pk2(o[dt][4 * g4] * inv, o[dt][4 * g4 + 1] * inv),
                                                             pk2(o[dt][4 * g4 + 2] * inv, o[dt][4 * g4 + 3] * inv)};
        }
    if (hh == 0) lse[(int64_t)bh * n + qq] = (mx + log2f(tot)) * AB_LN2;
}

template <int D>
static void attnb_launch(const u16* q, const u16* k, const u16* v, int64_t batch, int heads, int64_t n, int64_t m,
                         int rsq, int rskv, int kv_shared, int ro, float scale, u16* out, float* lse, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>((n + AB_WB - 1) / AB_WB), static_cast<unsigned>(batch * heads));
    launch(0, k_attnb_fwd<D>, grid, dim3(kBlock), s, q, k, v, static_cast<int>(n), static_cast<int>(m), heads, rsq,
           rskv, kv_shared, ro, scale * AB_LOG2E, out, lse);
}

// ---------------------------------------------------------------------------------------------
// Attention VJP on bf16 MFMAs (FlashAttention-2 recurrence, P never in HBM): delta = rowsum(dO o O),
// then
//   k_attnb_dq   per wave 32 queries: S^T = K Q^T, dP^T = V dO^T (Q^T, dO^T in registers), dS^T =
//                P^T (dP^T - delta), dQ^T += K^T dS^T (K^T staged in LDS in the C layout's key order)
//   k_attnb_dkv  per wave 32 keys: S = Q K^T, dP = dO V^T (K^T, V^T in registers), dS = P (dP -
//                delta), dV^T += dO^T P and dK^T += Q^T dS (Q^T, dO^T staged in that order)
// P and dS are rounded to bf16 as MFMA operands (as the forward's P); fp32 accumulation.
// ---------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kBlock) void k_attnb_delta(const u16* __restrict__ out, const u16* __restrict__ dout,
                                                        int n, int heads, int ro, int64_t rows,
                                                        float* __restrict__ delta) {
    const int64_t rr = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (rr >= rows) return;
    const int bh = static_cast<int>(rr / n), i = static_cast<int>(rr - (int64_t)bh * n);
    const int b = bh / heads, hd = bh - b * heads;
    const int64_t off = ((int64_t)b * n + i) * ro + hd * D;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < D / 8; ++j) {
        float a[8], c[8];
        unpack8(*reinterpret_cast<const bq_u4*>(out + off + 8 * j), a);
        unpack8(*reinterpret_cast<const bq_u4*>(dout + off + 8 * j), c);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = fmaf(a[e], c[e], acc);
    }
    delta[rr] = acc;
}

// the B-operand fragments of 32 rows (lane row r) of a row-major [rows][D] operand, d padded to 16
template <int D>
__device__ __forceinline__ void ab_rowfrags(const u16* __restrict__ src, int64_t rs, int row, int limit, int hh,
                                            bq_u4 (&f)[AbGeo<D>::DK]) {
#pragma unroll
    for (int s = 0; s < AbGeo<D>::DK; ++s) {
        const int d0 = 16 * s + 8 * hh;
        f[s] = (d0 + 8 <= D && row < limit) ? *reinterpret_cast<const bq_u4*>(src + (int64_t)row * rs + d0)
                                            : bq_u4{0u, 0u, 0u, 0u};
    }
}

template <int D>
__device__ __forceinline__ void ab_zero_pad(u16* img) {
    using G = AbGeo<D>;
    if constexpr (G::DKP > D) {
        for (int i = threadIdx.x; i < G::SB; i += kBlock)
#pragma unroll
            for (int cc = D; cc < G::DKP; cc += 2) *reinterpret_cast<unsigned*>(img + i * G::KROW + cc) = 0u;
    }
}

// C-layout rows d of 32 columns -> bf16 row-major output: lane's column `row`, 4 d per store
template <int D>
__device__ __forceinline__ void ab_store_rows(u16* __restrict__ dst, int64_t rs, int row, int limit, int hh,
                                              const bq_f16 (&acc)[AbGeo<D>::DT], float mul) {
    if (row >= limit) return;
    u16* o = dst + (int64_t)row * rs;
#pragma unroll
    for (int dt = 0; dt < AbGeo<D>::DT; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int d0 = 32 * dt + 8 * g4 + 4 * hh;
            if (d0 + 4 <= D)
                *reinterpret_cast<bq_u2*>(o + d0) = bq_u2{pk2(acc[dt][4 * g4] * mul, acc[dt][4 * g4 + 1] * mul),
                                                          pk2(acc[dt][4 * g4 + 2] * mul, acc[dt][4 * g4 + 3] * mul)};
        }
}

template <int D>
__global__ __launch_bounds__(kBlock) void k_attnb_dq(const u16* __restrict__ q, const u16* __restrict__ k,
                                                     const u16* __restrict__ v, const u16* __restrict__ dout,
                                                     const float* __restrict__ lse, const float* __restrict__ delta,
                                                     int n, int m, int heads, int rsq, int rskv, int kv_shared,
                                                     int ro, int rdq, float sl2, float scale,
                                                     u16* __restrict__ dq) {
    using G = AbGeo<D>;
    __shared__ __attribute__((aligned(16))) u16 Kn[G::IMG];
    __shared__ __attribute__((aligned(16))) u16 Vn[G::IMG];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int bh = blockIdx.y, b = bh / heads, hd = bh - b * heads;
    const int qq = blockIdx.x * AB_WB + wv * AB_QW + r;
    const int64_t kvb = (kv_shared ? 0 : (int64_t)b * m * rskv) + hd * D;
    ab_zero_pad<D>(Kn);
    ab_zero_pad<D>(Vn);
    const u16* trk = Kn + ab_trlane(lane, G::KROW);
    bq_u4 qf[G::DK], of[G::DK];
    ab_rowfrags<D>(q + (int64_t)b * n * rsq + hd * D, rsq, qq, n, hh, qf);
    ab_rowfrags<D>(dout + (int64_t)b * n * ro + hd * D, ro, qq, n, hh, of);
    const float ll = qq < n ? lse[(int64_t)bh * n + qq] * AB_LOG2E : 0.f;
    const float dl = qq < n ? delta[(int64_t)bh * n + qq] : 0.f;
    bq_f16 acc[G::DT];
#pragma unroll
    for (int dt = 0; dt < G::DT; ++dt) acc[dt] = bq_f16{};
    const int nst = (m + G::SB - 1) / G::SB;
    bq_u4 ks[G::NVU][2], vs[G::NVU][2];
    ab_ld_pairs<D>(k + kvb, rskv, 0, m, ks);
    ab_ld_pairs<D>(v + kvb, rskv, 0, m, vs);
    for (int si = 0; si < nst; ++si) {
        __syncthreads();
        ab_st_nat<D>(Kn, ks);
        ab_st_nat<D>(Vn, vs);
        __syncthreads();
        if (si + 1 < nst) {
            ab_ld_pairs<D>(k + kvb, rskv, (si + 1) * G::SB, m, ks);
            ab_ld_pairs<D>(v + kvb, rskv, (si + 1) * G::SB, m, vs);
        }
        const int kbase = si * G::SB;
#pragma unroll
        for (int kb32 = 0; kb32 < G::SB / 32; ++kb32) {
            if (kbase + kb32 * 32 >= m) break;
            bq_f16 sv = bq_f16{}, dp = bq_f16{};
#pragma unroll
            for (int s2 = 0; s2 < G::DK; ++s2) {
                const int o = (kb32 * 32 + r) * G::KROW + 16 * s2 + 8 * hh;
                sv = bq_mfma(*reinterpret_cast<const bq_u4*>(Kn + o), qf[s2], sv);
                dp = bq_mfma(*reinterpret_cast<const bq_u4*>(Vn + o), of[s2], dp);
            }
            float ds[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = kbase + kb32 * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh;
                const float p = key < m ? __builtin_amdgcn_exp2f(fmaf(sv[i], sl2, -ll)) : 0.f;
                ds[i] = p * (dp[i] - dl);
            }
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const bq_u4 pf = {pk2(ds[8 * kk], ds[8 * kk + 1]), pk2(ds[8 * kk + 2], ds[8 * kk + 3]),
                                  pk2(ds[8 * kk + 4], ds[8 * kk + 5]), pk2(ds[8 * kk + 6], ds[8 * kk + 7])};
#pragma unroll
                for (int dt = 0; dt < G::DT; ++dt) {
                    const bq_u4 a = ab_tr<G::KROW>(trk, (kb32 * 32 + kk * 16) * G::KROW + 32 * dt);
                    acc[dt] = bq_mfma(a, pf, acc[dt]);
                }
            }
        }
    }
    ab_store_rows<D>(dq + (int64_t)b * n * rdq + hd * D, rdq, qq, n, hh, acc, scale);
}

template <int D>
__global__ __launch_bounds__(kBlock) void k_attnb_dkv(const u16* __restrict__ q, const u16* __restrict__ k,
                                                      const u16* __restrict__ v, const u16* __restrict__ dout,
                                                      const float* __restrict__ lse, const float* __restrict__ delta,
                                                      int n, int heads, int rs, int ro, int rdkv, float sl2,
                                                      float scale, u16* __restrict__ dk, u16* __restrict__ dv) {
    using G = AbGeo<D>;
    __shared__ __attribute__((aligned(16))) u16 Qn[G::IMG];
    __shared__ __attribute__((aligned(16))) u16 On[G::IMG];
    __shared__ __attribute__((aligned(16))) float Ls[G::SB], Dl[G::SB];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int bh = blockIdx.y, b = bh / heads, hd = bh - b * heads;
    const int kk_ = blockIdx.x * AB_WB + wv * AB_QW + r;  // this lane's key
    const int64_t base = (int64_t)b * n * rs + hd * D, obase = (int64_t)b * n * ro + hd * D;
    ab_zero_pad<D>(Qn);
    ab_zero_pad<D>(On);
    const u16* trq = Qn + ab_trlane(lane, G::KROW);
    const u16* tro = On + ab_trlane(lane, G::KROW);
    bq_u4 kf[G::DK], vf[G::DK];
    ab_rowfrags<D>(k + base, rs, kk_, n, hh, kf);
    ab_rowfrags<D>(v + base, rs, kk_, n, hh, vf);
    bq_f16 ak[G::DT], av[G::DT];
#pragma unroll
    for (int dt = 0; dt < G::DT; ++dt) ak[dt] = bq_f16{}, av[dt] = bq_f16{};
    const int nst = (n + G::SB - 1) / G::SB;
    bq_u4 qs[G::NVU][2], os[G::NVU][2];
    // the row constants of the next stage: a plain load in flight beside the Q / dO rows (any
    // arithmetic on it here would make the compiler wait for every load of the stage at once);
    // scaled and masked when stored
    float lv = 0.f;
    auto ld = [&](int si) {
        ab_ld_pairs<D>(q + base, rs, si * G::SB, n, qs);
        ab_ld_pairs<D>(dout + obase, ro, si * G::SB, n, os);
        const int qi = min(si * G::SB + (tid & (G::SB - 1)), n - 1);
        lv = ((tid & G::SB) ? delta : lse)[(int64_t)bh * n + qi];  // every thread: no branch
    };
    ld(0);
    for (int si = 0; si < nst; ++si) {
        __syncthreads();
        ab_st_nat<D>(Qn, qs);
        ab_st_nat<D>(On, os);
        {
            const bool in = si * G::SB + (tid & (G::SB - 1)) < n;
            if (tid < G::SB)
                Ls[tid] = in ? lv * AB_LOG2E : INFINITY;
            else if (tid < 2 * G::SB)
                Dl[tid - G::SB] = in ? lv : 0.f;
        }
        __syncthreads();
        if (si + 1 < nst) ld(si + 1);
#pragma unroll
        for (int ib32 = 0; ib32 < G::SB / 32; ++ib32) {
            if (si * G::SB + ib32 * 32 >= n) break;
            bq_f16 sv = bq_f16{}, dp = bq_f16{};
#pragma unroll
            for (int s2 = 0; s2 < G::DK; ++s2) {
                const int o = (ib32 * 32 + r) * G::KROW + 16 * s2 + 8 * hh;
                sv = bq_mfma(*reinterpret_cast<const bq_u4*>(Qn + o), kf[s2], sv);
                dp = bq_mfma(*reinterpret_cast<const bq_u4*>(On + o), vf[s2], dp);
            }
            float p[16], ds[16];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int q0 = ib32 * 32 + 8 * g + 4 * hh;
                const float4 l4 = *reinterpret_cast<const float4*>(Ls + q0);
                const float4 d4 = *reinterpret_cast<const float4*>(Dl + q0);
                const float la[4] = {l4.x, l4.y, l4.z, l4.w}, da[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 4 * g + e;
                    p[i] = __builtin_amdgcn_exp2f(fmaf(sv[i], sl2, -la[e]));
                    ds[i] = p[i] * (dp[i] - da[e]);
                }
            }
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const bq_u4 pp = {pk2(p[8 * kk], p[8 * kk + 1]), pk2(p[8 * kk + 2], p[8 * kk + 3]),
                                  pk2(p[8 * kk + 4], p[8 * kk + 5]), pk2(p[8 * kk + 6], p[8 * kk + 7])};
                const bq_u4 pd = {pk2(ds[8 * kk], ds[8 * kk + 1]), pk2(ds[8 * kk + 2], ds[8 * kk + 3]),
                                  pk2(ds[8 * kk + 4], ds[8 * kk + 5]), pk2(ds[8 * kk + 6], ds[8 * kk + 7])};
#pragma unroll
                for (int dt = 0; dt < G::DT; ++dt) {
                    const int o = (ib32 * 32 + kk * 16) * G::KROW + 32 * dt;
                    av[dt] = bq_mfma(ab_tr<G::KROW>(tro, o), pp, av[dt]);
                    ak[dt] = bq_mfma(ab_tr<G::KROW>(trq, o), pd, ak[dt]);
                }
            }
        }
    }
    ab_store_rows<D>(dk + (int64_t)b * n * rdkv + hd * D, rdkv, kk_, n, hh, ak, scale);
    ab_store_rows<D>(dv + (int64_t)b * n * rdkv + hd * D, rdkv, kk_, n, hh, av, 1.f);
}

template <int D>
static void attnb_bwd_launch(const u16* q, const u16* k, const u16* v, const u16* out, const u16* dout,
                             const float* lse, int64_t batch, int heads, int64_t n, int64_t m, int rsq, int rskv,
                             int kv_shared, int ro, int rdq, int rdkv, float scale, float* delta, u16* dq, u16* dk,
                             u16* dv, hipStream_t s) {
    const int64_t rows = batch * heads * n;
    launch(0, k_attnb_delta<D>, dim3(static_cast<unsigned>((rows + kBlock - 1) / kBlock)), dim3(kBlock), s, out, dout,
           static_cast<int>(n), heads, ro, rows, delta);
    const float sl2 = scale * AB_LOG2E;
    if (dq)
        launch(0, k_attnb_dq<D>, dim3(static_cast<unsigned>((n + AB_WB - 1) / AB_WB), static_cast<unsigned>(batch * heads)),
               dim3(kBlock), s, q, k, v, dout, lse, static_cast<const float*>(delta), static_cast<int>(n),
               static_cast<int>(m), heads, rsq, rskv, kv_shared, ro, rdq, sl2, scale, dq);
    if (dk)
        launch(0, k_attnb_dkv<D>, dim3(static_cast<unsigned>((n + AB_WB - 1) / AB_WB), static_cast<unsigned>(batch * heads)),
               dim3(kBlock), s, q, k, v, dout, lse, static_cast<const float*>(delta), static_cast<int>(n), heads, rsq,
               ro, rdkv, sl2, scale, dk, dv);
}

}  // namespace sp

using namespace sp;

extern "C" {

// ---- attention ------------------------------------------------------------------------------

int sp_attention_bf16_supported(int64_t batch, int32_t heads, int64_t n, int64_t m, int32_t d) {
    if (batch <= 0 || heads <= 0 || batch * heads > 65535 || n <= 0 || m <= 0 || n > (int64_t(1) << 24) ||
        m > (int64_t(1) << 24))
        return 0;
    return d == 40 || d == 64 || d == 80 || d == 160;
}

// out[b][i][h d .. h d + d) = softmax(q k^T scale) v for head h: q rows of stride rsq
// ([batch][n][rsq]), k / v rows of stride rskv ([batch or 1 (kv_shared)][m][rskv]), out rows of
// stride ro; bf16 in and out, lse [batch heads][n] fp32 (natural log).  Pointers at head 0.
int sp_attention_bf16_fwd(const void* q, const void* k, const void* v, int64_t batch, int32_t heads, int64_t n,
                          int64_t m, int32_t d, int32_t rsq, int32_t rskv, int32_t kv_shared, int32_t ro, float scale,
                          void* out, float* lse, sp_stream_t stream) {
    if (!q || !k || !v || !out || !lse || !sp_attention_bf16_supported(batch, heads, n, m, d)) return SP_EINVAL;
    if (rsq < heads * d || rskv < heads * d || ro < heads * d || rsq % 8 || rskv % 8 || ro % 4) return SP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const u16* qq = static_cast<const u16*>(q);
    const u16* kk = static_cast<const u16*>(k);
    const u16* vv = static_cast<const u16*>(v);
    u16* oo = static_cast<u16*>(out);
    switch (d) {
        case 40: attnb_launch<40>(qq, kk, vv, batch, heads, n, m, rsq, rskv, kv_shared, ro, scale, oo, lse, s); break;
        case 64: attnb_launch<64>(qq, kk, vv, batch, heads, n, m, rsq, rskv, kv_shared, ro, scale, oo, lse, s); break;
        case 80: attnb_launch<80>(qq, kk, vv, batch, heads, n, m, rsq, rskv, kv_shared, ro, scale, oo, lse, s); break;
        default: attnb_launch<160>(qq, kk, vv, batch, heads, n, m, rsq, rskv, kv_shared, ro, scale, oo, lse, s); break;
    }
    return check_launch("sp_attention_bf16_fwd");
}

// VJP of sp_attention_bf16_fwd given its output and lse: delta [batch heads][n] fp32 (caller's
// scratch); dq rows of stride rdq ([batch][n][rdq]); dk / dv (self-attention only: m == n, one K/V
// per sample, rsq == rskv) rows of stride rdkv, or NULL (cross-attention: the context is constant).
int sp_attention_bf16_bwd_supported(int64_t batch, int32_t heads, int64_t n, int64_t m, int32_t d) {
    return sp_attention_bf16_supported(batch, heads, n, m, d) && (d == 40 || d == 64 || d == 80);
}

int sp_attention_bf16_bwd(const void* q, const void* k, const void* v, const void* out, const void* dout,
                          const float* lse, int64_t batch, int32_t heads, int64_t n, int64_t m, int32_t d,
                          int32_t rsq, int32_t rskv, int32_t kv_shared, int32_t ro, int32_t rdq, int32_t rdkv,
                          float scale, float* delta, void* dq, void* dk, void* dv, sp_stream_t stream) {
    if (!q || !k || !v || !out || !dout || !lse || !delta || !sp_attention_bf16_bwd_supported(batch, heads, n, m, d))
        return SP_EINVAL;
    if (rsq < heads * d || rskv < heads * d || ro < heads * d || rsq % 8 || rskv % 8 || ro % 8 || rdq % 4 || rdkv % 4)
        return SP_EINVAL;
    if ((dk || dv) && (!dk || !dv || m != n || kv_shared || rsq != rskv || rdkv < heads * d)) return SP_EINVAL;
    if (dq && rdq < heads * d) return SP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const u16 *qq = static_cast<const u16*>(q), *kk = static_cast<const u16*>(k), *vv = static_cast<const u16*>(v);
    const u16 *oo = static_cast<const u16*>(out), *dd = static_cast<const u16*>(dout);
    u16 *a = static_cast<u16*>(dq), *bb = static_cast<u16*>(dk), *c = static_cast<u16*>(dv);
    switch (d) {
        case 40: attnb_bwd_launch<40>(qq, kk, vv, oo, dd, lse, batch, heads, n, m, rsq, rskv, kv_shared, ro, rdq, rdkv, scale, delta, a, bb, c, s); break;
        case 64: attnb_bwd_launch<64>(qq, kk, vv, oo, dd, lse, batch, heads, n, m, rsq, rskv, kv_shared, ro, rdq, rdkv, scale, delta, a, bb, c, s); break;
        default: attnb_bwd_launch<80>(qq, kk, vv, oo, dd, lse, batch, heads, n, m, rsq, rskv, kv_shared, ro, rdq, rdkv, scale, delta, a, bb, c, s); break;
    }
    return check_launch("sp_attention_bf16_bwd");
}

}  // extern "C"
