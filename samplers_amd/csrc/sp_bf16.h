// The priors at the reference's reduced precision (scripts/run_psld.py:14-20 runs SD 1.5 in bf16;
// stable_diffusion.py:90-101 / ddpm.py:23-34 take any torch_dtype): bf16 activations in HBM,
// bf16 operands on the bf16 MFMAs, fp32 accumulation and fp32 statistics.
//
// Layout: channels-last (NHWC) activations.  The 3x3 convolution is an implicit GEMM whose
// contraction runs over (tap, input channel); with the channels innermost, the eight channels a
// lane feeds to one MFMA are 16 contiguous bytes of one pixel, so the input patch is staged
// into LDS as [pixel][16 channels] rows and every MFMA operand is one ds_read_b128 — no
// transposes anywhere (NCHW would put the contraction index at a stride of H*W).  The same
// layout is the token layout of the transformer blocks ([b][h w][c]).
//
// One source file per kernel family, this header for what more than one of them uses:
//   sp_bf16_conv.hip       k_conv3x3_bf16<TC>, k_conv_reduce, k_pool2x2_bf16
//   sp_bf16_groupnorm.hip  k_gnb_stats / _final / _apply / _bwd_*
//   sp_bf16_rows.hip       GEGLU and LayerNorm over token rows
//   sp_bf16_attention.hip  k_attnb_fwd<D>, k_attnb_delta / _dq / _dkv
//
// C layout of v_mfma_f32_32x32x16_bf16: register i of lane l is row (i&3) + 8(i>>2) + 4(l>>5),
// column l&31; A/B fragments: lane l holds A[row l&31][k 8(l>>5) + j] / B[k 8(l>>5) + j][col l&31],
// j = 0..7 (cdna_hip_programming.md §3).
#pragma once

#include "sp_common.h"

#include <algorithm>
#include <cmath>

namespace sp {

typedef float bq_f16 __attribute__((ext_vector_type(16)));
typedef unsigned bq_u4 __attribute__((ext_vector_type(4)));
typedef unsigned bq_u2 __attribute__((ext_vector_type(2)));
typedef __bf16 bq_bf8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16;

#ifndef BQ_EXP
#define BQ_EXP 0  // diagnostics only: 7 = each 32x32x16 MFMA replaced by two 16x16x32 ones on the same
                  // operands (the same MACs, wrong results): the clock the chip holds per MFMA shape;
                  // 8 = the TC = 32 conv's fragment reads after tap 0 removed (wrong results);
                  // 9 = its global loads after the first two stages removed (wrong results);
                  // 10 = every patch load from one cached line (weights as usual; wrong results)
#endif
__device__ __forceinline__ bq_f16 bq_mfma(bq_u4 a, bq_u4 b, bq_f16 c) {
#if BQ_EXP == 7
    typedef float bq_f4 __attribute__((ext_vector_type(4)));
    bq_f4 c0 = {c[0], c[1], c[2], c[3]}, c1 = {c[4], c[5], c[6], c[7]};
    c0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bq_bf8, a), __builtin_bit_cast(bq_bf8, b), c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bq_bf8, b), __builtin_bit_cast(bq_bf8, a), c1, 0, 0, 0);
    c[0] = c0[0], c[1] = c0[1], c[2] = c0[2], c[3] = c0[3], c[4] = c1[0], c[5] = c1[1], c[6] = c1[2], c[7] = c1[3];
    return c;
#else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bq_bf8, a), __builtin_bit_cast(bq_bf8, b), c,
                                                   0, 0, 0);
#endif
}

__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ float bf1(u16 v) { return __uint_as_float(static_cast<unsigned>(v) << 16); }
// round to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ u16 f2bf(float f) { return __builtin_bit_cast(u16, static_cast<__bf16>(f)); }
__device__ __forceinline__ unsigned pk2(float a, float b) {
    return static_cast<unsigned>(f2bf(a)) | (static_cast<unsigned>(f2bf(b)) << 16);
}
__device__ __forceinline__ void unpack8(bq_u4 v, float (&f)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) f[2 * i] = bf_lo(v[i]), f[2 * i + 1] = bf_hi(v[i]);
}
__device__ __forceinline__ bq_u4 pack8(const float (&f)[8]) {
    return bq_u4{pk2(f[0], f[1]), pk2(f[2], f[3]), pk2(f[4], f[5]), pk2(f[6], f[7])};
}
// static: sp_groupnorm.hip has an sp::silu_f of its own with another body (an exact sigmoid)
static __device__ __forceinline__ float silu_f(float y) { return y * __builtin_amdgcn_rcpf(1.f + __expf(-y)); }
__device__ __forceinline__ void ld8f(const float* p, float (&f)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    f[0] = a.x, f[1] = a.y, f[2] = a.z, f[3] = a.w, f[4] = b.x, f[5] = b.y, f[6] = b.z, f[7] = b.w;
}

// grid.x of the streaming kernels (one 16-byte vector per thread-iteration)
static inline unsigned stream_blocks(int64_t vectors) {
    return static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>((vectors + kBlock - 1) / kBlock, 256 * 16)));
}

// The GroupNorm a conv launch's epilogue serves (k_conv3x3_bf16's GS / FS; sp_bf16_conv.hip)
struct ConvGn {
    const u16* x1;
    const u16* x2;
    int c1, act;
    const float* co;
    const float* gamma;
    float* part;
};

// The GroupNorm passes (sp_bf16_groupnorm.hip), one launch each, for the sp_groupnorm_bf16* entries
// and the fused conv + GroupNorm entries of sp_bf16_conv.hip (a kernel is launched from the file
// that defines it).  x1 / x2: the c1 + c2 concatenated channels; the chunked passes (stats, apply,
// bwd_apply) take their grid from (n, c1 + c2, hw); act / nt pick the kernel's ACT / NT.
void gnb_coefs_pass(const float* stats, const float* cbias, const float* gamma, const float* beta, int64_t n, int c,
                    int groups, float* co, hipStream_t s);
// mode 0: forward shifted sums (dz, co, gamma unused); 1: the VJP's sums.  part [n][chunks][2][c]
void gnb_stats_pass(int mode, bool act, bool nt, const u16* x1, const u16* x2, int c1, int c2, const float* cbias,
                    const u16* dz, const float* co, const float* gamma, int64_t n, int64_t hw, float* part,
                    hipStream_t s);
void gnb_final_fwd_pass(const u16* x1, const u16* x2, int c1, int c2, const float* cbias, const float* part, int chunks,
                        int64_t n, int64_t hw, int groups, float eps, const float* gamma, const float* beta,
                        float* stats, float* co, hipStream_t s);
// part [n][tiles][3][c] from the FS conv epilogue, px pixels per tile
void gnb_final_fwd_tiles_pass(const float* part, int tiles, int64_t px, int64_t n, int64_t hw, int c, int groups,
                              float eps, const float* cbias, const float* gamma, const float* beta, float* stats,
                              float* co, hipStream_t s);
void gnb_final_bwd_pass(const float* part, int chunks, int64_t n, int64_t hw, int c, int groups, const float* stats,
                        const float* gamma, const float* co, float* co2, hipStream_t s);
void gnb_apply_pass(bool act, bool nt, const u16* x1, const u16* x2, int c1, int c2, const float* co, int64_t n,
                    int64_t hw, u16* z, int z_layout, hipStream_t s);
void gnb_bwd_apply_pass(bool act, bool nt, const u16* dz, const u16* x1, const u16* x2, int c1, int c2,
                        const float* co, const float* co2, int64_t n, int64_t hw, u16* dx1, u16* dx2,
                        const u16* add1, const u16* add2, const u16* add1b, int dx_layout, hipStream_t s);

}  // namespace sp
