// In-LDS Stockham FFT core shared by the kinds that transform in LDS (sp_phase.hip,
// sp_psf_fft.hip; the algorithm and the LDS layout are described in sp_phase.hip's file comment),
// and at the end the one host helper, fft_stage, through which those kinds launch.  Internal; include after sp_ops.h, inside a translation unit that defines SP_TU.
#pragma once

#include "sp_ops.h"

namespace sp {

// bytes of dynamic LDS a workgroup may take: five workgroups per CU.  Measured at B = 64,
// 3 x 256^2 -> 384^2 (pass 1, us): 8 lines per workgroup (62 KB) 812, 7 lines 665, 5 lines 607,
// 4 lines (29 KB) 573, 3 lines 605 - resident waves hide the barrier of every pass.
constexpr int kPhaseLds = 32000;
constexpr int kPhaseMaxLines = 16;

__host__ __device__ inline int phase_np(int N) { return (N + (N >> 4)) | 1; }
__host__ __device__ inline int phase_slot(int q) { return q + (q >> 4); }

// lines of an N-point transform per workgroup (a launch parameter, computed on the host)
static inline int phase_lines(int N) {
    int t = (kPhaseLds - 8 * N) / (16 * phase_np(N));
    if (t > kPhaseMaxLines) t = kPhaseMaxLines;
    return t < 1 ? 1 : t;
}

static inline int phase_lds_bytes(int N) { return 8 * N + 16 * phase_lines(N) * phase_np(N); }

// 2^k or 3 * 2^k in [8, 1024]
static bool phase_size_ok(int N) {
    if (N < 8 || N > 1024) return false;
    while (N % 2 == 0) N /= 2;
    return N == 1 || N == 3;
}

__device__ __forceinline__ float2 cmul(float2 a, float2 w) {
    return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// tw[q] = exp(-2 pi i q / N), q < N
__device__ __forceinline__ void phase_twiddles(float2* tw, int N) {
    for (int q = threadIdx.x; q < N; q += kBlock) {
        double s, c;
        sincospi(-2.0 * (double)q / (double)N, &s, &c);
        tw[q] = make_float2((float)c, (float)s);
    }
}

// one Stockham pass of radix R over T lines (file comment); Ns is a power of two
template <int R>
__device__ __forceinline__ void phase_pass(const float2* __restrict__ in, float2* __restrict__ out,
                                           const float2* __restrict__ tw, int N, int NP, int T,
                                           int Ns, bool inverse) {
    const int M = N / R, total = T * M, step = N / (Ns * R);
    const int dq = kBlock / M, dr = kBlock - dq * M;
    int t = static_cast<int>(threadIdx.x) / M, j = static_cast<int>(threadIdx.x) - t * M;
    for (int idx = threadIdx.x; idx < total; idx += kBlock) {
        SP_DCHECK(t < T && j < M && t * M + j == idx);
        const int k = j & (Ns - 1);
        const float2* li = in + t * NP;
        float2 v[R];
#pragma unroll
        for (int i = 0; i < R; ++i) v[i] = li[phase_slot(j + i * M)];
        if (Ns > 1) {  // the first pass has k = 0: every twiddle is 1
#pragma unroll
            for (int i = 1; i < R; ++i) {
                SP_DCHECK(i * k * step < N);
                float2 w = tw[i * k * step];
                if (inverse) w.y = -w.y;
                v[i] = cmul(v[i], w);
            }
        }
        float2 o[R];
        if constexpr (R == 2) {
            o[0] = cadd(v[0], v[1]);
            o[1] = csub(v[0], v[1]);
        } else if constexpr (R == 4) {
            const float2 a0 = cadd(v[0], v[2]), a1 = csub(v[0], v[2]), a2 = cadd(v[1], v[3]);
            const float2 d = csub(v[1], v[3]);
            const float2 a3 = inverse ? make_float2(-d.y, d.x) : make_float2(d.y, -d.x);  // +-i d
            o[0] = cadd(a0, a2);
            o[1] = cadd(a1, a3);
            o[2] = csub(a0, a2);
            o[3] = csub(a1, a3);
        } else {
            constexpr float c = 0.86602540378443864676f;  // sqrt(3) / 2
            const float2 s = cadd(v[1], v[2]), d = csub(v[1], v[2]);
            const float2 m = make_float2(v[0].x - 0.5f * s.x, v[0].y - 0.5f * s.y);
            const float2 e = inverse ? make_float2(-c * d.y, c * d.x) : make_float2(c * d.y, -c * d.x);
            o[0] = cadd(v[0], s);
            o[1] = cadd(m, e);
            o[2] = csub(m, e);
        }
        const int j0 = (j - k) * R + k;
        float2* lo = out + t * NP;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            SP_DCHECK(j0 + i * Ns < N && phase_slot(j0 + i * Ns) < NP);
            lo[phase_slot(j0 + i * Ns)] = o[i];
        }
        t += dq, j += dr;
        if (j >= M) j -= M, ++t;
    }
    __syncthreads();
}

// N-point transforms of the T lines in `a` (natural order in, natural order out); returns the
// buffer that holds the result.  The caller has synchronised after filling `a` and `tw`.
__device__ __forceinline__ float2* phase_fft(float2* a, float2* b, const float2* tw, int N, int NP,
                                             int T, bool inverse) {
    const bool three = N % 3 == 0;
    const int pow2 = three ? N / 3 : N;
    int Ns = 1;
    while (Ns < pow2) {
        if ((pow2 / Ns) % 4 == 0) {
            phase_pass<4>(a, b, tw, N, NP, T, Ns, inverse);
            Ns *= 4;
        } else {
            phase_pass<2>(a, b, tw, N, NP, T, Ns, inverse);
            Ns *= 2;
        }
        float2* s = a;
        a = b, b = s;
    }
    if (three) {
        phase_pass<3>(a, b, tw, N, NP, T, Ns, inverse);
        a = b;
    }
    return a;
}

// ---------------------------------------------------------------------------
// host side: how every kind launches a stage of N-point transforms
// ---------------------------------------------------------------------------
// typed nulls for the kernel arguments a stage does not use
constexpr const float* kNoIn = nullptr;
constexpr float* kNoOut = nullptr;
constexpr const sp_step_rec* kNoSched = nullptr;
constexpr const int32_t* kNoCursor = nullptr;

// `gx` workgroups per sample of `kernel` on N-point transforms (phase_lds_bytes(N) of dynamic
// LDS), reported under the entry point `what`; kind / work as launch_w (kind 0: untimed); the
// kernel's own arguments follow, phase_lines(N) among them
template <typename K, typename... Args>
static inline int fft_stage(const char* what, int kind, double work, K kernel, int64_t gx,
                            int64_t batch, int N, hipStream_t s, Args... args) {
    launch_w(kind, work, kernel, sample_grid(gx, batch), dim3(kBlock), (size_t)phase_lds_bytes(N), s,
             args...);
    return check_launch(what);
}

}  // namespace sp
