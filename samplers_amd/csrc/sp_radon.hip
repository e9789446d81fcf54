// Parallel-beam CT projector (SP_OP_RADON): Joseph's method, depthwise over channel planes, unit
// pixel and detector spacing (the reference has no tomography operator; semantics in
// operators/radon.py, pinned in fp64 by tests/radon_ref.py).  x is (C, H, W), y is
// (C, n_angles, D); op.radius = n_angles, op.factor = D, op.taps = n_angles rows of
// (alpha, beta, length, axis).  With s0 = (D-1)/2, i0 = (H-1)/2, j0 = (W-1)/2 and, for axis 0,
// the dominant index d = i (cross index j, centres d0 = i0, x0 = j0), for axis 1 d = j (cross
// index i, d0 = j0, x0 = i0):
//   c(d, s)  = alpha (s - s0) + (beta (d - d0) + x0)               radon_pos, fp32, this order
//   y[a][s]  = length * sum_d [(1 - f) x[d, floor c] + f x[d, floor c + 1]],  f = c - floor c
// with 0 for a cross index off the image.  A^T is the exact transpose as a gather per pixel.
// Both kernels get their weights from radon_pos / radon_weights, written with __fadd_rn /
// __fsub_rn and radon_mul, a product the compiler cannot contract into the addition that
// consumes it (the toolchain's __fmul_rn is a plain multiply: left to itself the compiler fused
// the position in backproject and not in project, and the weights differed in the last bit).
// So the weights of A and A^T are the same fp32 numbers and only the order of summation differs.
//
// project: one workgroup owns one (plane, angle, chunk of <= 256 adjacent rays), one thread one
// ray, and sums its ray over d = 0 .. ND-1 in that order.  The dominant axis is swept in bands
// of 32.  The pixels a band of the chunk can touch are a slab of cross indices [xlo, xhi], found
// from radon_pos at the four corners (d, s) of the band (the rounded operations are monotone in
// d and in s, so every ray of the chunk stays inside).  The slab is staged in LDS as
// L[cross - xlo][d - db] with a pitch of 33 floats, x0 = (x - k eps) / a formed once per staged
// element, zeros off the image.  Staging is coalesced on either axis: along the cross index for
// axis 0 (an image row), along d for axis 1 (32-float row segments: the transposed staging, so
// the column-strided angles never gather from global memory).  A thread then reads 2 values
// per step; lanes are adjacent rays, whose cross indices differ by floor(alpha k): distinct
// slab rows, 33 banks apart, at most two lanes per bank.  A slab wider than the 400 staged rows
// (|alpha| > ~1.5, outside what radon_table makes) is gathered from global memory instead, with
// the same arithmetic per term, so both paths give the same bits; a band whose slab misses the
// image is skipped (its terms are all +0).
//
// backproject: one thread per pixel, lanes along W, angles in order.  Per angle the rays that
// can touch pixel (i, j) are within 1/|alpha| <= 1 of s* = s0 + ((x - x0) - beta (d - d0)) / alpha;
// the thread evaluates radon_pos for three candidates around floor(s*), without a branch, and
// keeps the weight (1 - f) where floor c is its cross index, f where floor c + 1 is, +0
// otherwise.  s* is only a locator.  A ray has a weight only if its fp32 position lies within 1
// of the pixel; the position is within 3 roundings at magnitudes < 2^11 (< 4e-4) of the exact
// one, which is alpha (s - s*) from the pixel, and the computed s* (hardware reciprocal) within
// 6e-4 of the exact one: so |s - s*| < 1 + 1e-3, and the candidates are floor(s*) and
// floor(s*) + 1, with floor(s*) - 1 only when s* - floor(s*) < 1/64 and floor(s*) + 2 only when
// it is > 63/64: the third evaluation is of that one (every load is clamped into the sinogram
// row, whatever s* is).  A sinogram plane is small and neighbouring pixels read neighbouring
// bins, so the gather runs out of L1 / L2.  No atomics.
//
// DPS pass 1 is two launches: `project` in residual mode writes work = grad_scale (y - A x0)
// and one |r|^2 partial per workgroup (block_sum's fixed order); `backproject` computes
// v = A^T work.  Nothing depends on the batch size, so a sample has the same bits in any batch.

#define SP_TU 19  // debug-build site numbering (sp_common.h SP_DCHECK)
#include "sp_ops.h"

namespace sp {

constexpr int RBD = 32;   // band depth along the dominant axis
constexpr int RPI = 33;   // LDS pitch of a slab row (odd: slab rows land on distinct banks)
constexpr int RXC = 400;  // slab rows staged at most (sqrt(2) * 255 + 31 + 3 = 395 for a real angle);
                          // 400 * 33 floats = 52.8 KB: three workgroups per CU
constexpr int RST = 4;    // steps of a ray whose LDS reads are in flight together
constexpr int RUN = 8;    // staged elements whose loads a thread keeps in flight
constexpr float RCLAMP = 1048576.f;  // positions are clamped here before the int conversion

enum { RADON_APPLY = 0, RADON_RESIDUAL = 1 };

// a * b rounded on its own: the empty asm hides the product from the contraction into a fused
// multiply-add with whatever addition consumes it (no instruction is emitted)
__device__ __forceinline__ float radon_mul(float a, float b) {
    float p = __fmul_rn(a, b);
    asm("" : "+v"(p));
    return p;
}

// the crossing position: the ONE function both kernels call (file comment)
__device__ __forceinline__ float radon_pos(float alpha, float beta, float ds, float dd, float off) {
    return __fadd_rn(radon_mul(alpha, ds), __fadd_rn(radon_mul(beta, dd), off));
}

// floor(c) as an int (clamped: a table outside its preconditions cannot overflow the conversion)
// and the two weights: w0 = 1 - f on floor(c), f on floor(c) + 1
__device__ __forceinline__ int radon_weights(float c, float& w0, float& f) {
    const float fl = floorf(c);
    f = __fsub_rn(c, fl);
    w0 = __fsub_rn(1.f, f);
    return static_cast<int>(fminf(fmaxf(fl, -RCLAMP), RCLAMP));
}

__device__ __forceinline__ int radon_floor(float c) {
    return static_cast<int>(floorf(fminf(fmaxf(c, -RCLAMP), RCLAMP)));
}

// one step of a ray's sum; the staged and the gathered path share it, so they share the bits
__device__ __forceinline__ float radon_step(float acc, float w0, float v0, float f, float v1) {
    return __fadd_rn(acc, __fadd_rn(radon_mul(w0, v0), radon_mul(f, v1)));
}

// x0 = (x - k eps) / a from loaded values (residual mode; 0, 0 -> 0 off the image), else x
template <int MODE>
__device__ __forceinline__ float radon_x0v(float xv, float ev, float a, float k) {
    if constexpr (MODE == RADON_RESIDUAL)
        return __fdiv_rn(__fsub_rn(xv, radon_mul(k, ev)), a);
    else
        return xv;
}

template <int MODE>
__device__ __forceinline__ float radon_x0(const float* __restrict__ x, const float* __restrict__ eps,
                                          int idx, float a, float k) {
    return radon_x0v<MODE>(x[idx], MODE == RADON_RESIDUAL ? eps[idx] : 0.f, a, k);
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void k_radon_project(sp_op op, const float* __restrict__ in,
                                                          const float* __restrict__ eps,
                                                          const float* __restrict__ y, int64_t y_div,
                                                          float a, float k, float gs,
                                                          float* __restrict__ out,
                                                          float* __restrict__ partial, int P,
                                                          int chunks, int rays,
                                                          const sp_step_rec* __restrict__ sched,
                                                          const int32_t* __restrict__ cursor) {
    __shared__ float L[RXC * RPI];
    __shared__ float red[4];
    if (MODE == RADON_RESIDUAL && sched) {  // device-resident schedule (graph replay)
        const sp_dps_coefs& cf = sched[*cursor].c;
        a = cf.a, k = cf.k, gs = cf.grad_scale;
    }
    const int H = op.height, W = op.width, C = op.channels, nA = op.radius, D = op.factor;
    const int tid = threadIdx.x;
    const int per_plane = nA * chunks;
    const int c = static_cast<int>(blockIdx.x) / per_plane;
    const int rem = static_cast<int>(blockIdx.x) - c * per_plane;
    const int ang = rem / chunks, chunk = rem - ang * chunks;
    const int64_t b = blockIdx.y;
    const int s_lo = chunk * rays, s_hi = min(D, s_lo + rays) - 1;  // the chunk's rays, inclusive
    const int s = s_lo + tid;
    const bool active = s <= s_hi;
    SP_DCHECK(c < C && ang < nA && s_lo <= s_hi && rays <= kBlock && static_cast<int>(blockIdx.x) < P);

    const float* __restrict__ row = op.taps + 4 * ang;
    const float alpha = row[0], beta = row[1], length = row[2];
    const bool axis = row[3] != 0.f;
    const int ND = axis ? W : H, NX = axis ? H : W;  // dominant / cross extent
    const int sd = axis ? 1 : W, sx = axis ? W : 1;  // their strides in the plane
    const float s0 = 0.5f * static_cast<float>(D - 1), d0 = 0.5f * static_cast<float>(ND - 1);
    const float off = 0.5f * static_cast<float>(NX - 1);
    const float ds = static_cast<float>(s) - s0;
    const float ds_lo = static_cast<float>(s_lo) - s0, ds_hi = static_cast<float>(s_hi) - s0;

    const int plane = H * W;  // < 2^31: in-plane offsets are 32-bit
    const int64_t poff = (b * C + c) * static_cast<int64_t>(plane);
    const float* __restrict__ ip = in + poff;
    const float* __restrict__ ep = MODE == RADON_RESIDUAL ? eps + poff : nullptr;

    float acc = 0.f;
    bool staged_before = false;
    for (int db = 0; db < ND; db += RBD) {
        const int nd = min(RBD, ND - db);
        // the slab of cross indices this band of the chunk can touch (workgroup-uniform)
        const float dd_lo = static_cast<float>(db) - d0, dd_hi = static_cast<float>(db + nd - 1) - d0;
        const float c00 = radon_pos(alpha, beta, ds_lo, dd_lo, off), c01 = radon_pos(alpha, beta, ds_lo, dd_hi, off);
        const float c10 = radon_pos(alpha, beta, ds_hi, dd_lo, off), c11 = radon_pos(alpha, beta, ds_hi, dd_hi, off);
        const int xlo = radon_floor(fminf(fminf(c00, c01), fminf(c10, c11)));
        const int xhi = radon_floor(fmaxf(fmaxf(c00, c01), fmaxf(c10, c11))) + 1;
        if (xhi < 0 || xlo >= NX) continue;  // the band misses the image: every term is +0
        const int XCn = xhi - xlo + 1;
        if (XCn <= RXC) {
            if (staged_before) __syncthreads();  // the previous band's reads are done
            staged_before = true;
            // a thread issues the loads of RUN staged elements before it uses the first: the
            // staging is bound by the latency of its loads, not by their number
            float xv[RUN], ev[RUN];
            if (!axis) {  // lanes along the cross index = along an image row
                for (int xc = tid; xc < XCn; xc += kBlock) {
                    const int gx = xlo + xc;
                    const bool in = gx >= 0 && gx < NX;
                    for (int dq = 0; dq < nd; dq += RUN) {
#pragma unroll
                        for (int u = 0; u < RUN; ++u) {
                            const bool ok = in && dq + u < nd;
                            const int idx = ok ? (db + dq + u) * sd + gx * sx : 0;
                            SP_DCHECK(idx >= 0 && idx < plane);
                            xv[u] = ok ? ip[idx] : 0.f;
                            ev[u] = (MODE == RADON_RESIDUAL && ok) ? ep[idx] : 0.f;
                        }
#pragma unroll
                        for (int u = 0; u < RUN; ++u)
                            if (dq + u < nd) {
                                SP_DCHECK(xc * RPI + dq + u < RXC * RPI);
                                L[xc * RPI + dq + u] = radon_x0v<MODE>(xv[u], ev[u], a, k);
                            }
                    }
                }
            } else {  // lanes along d = along an image row again: 32-float segments, transposed
                const int total = XCn * RBD;
                for (int e0 = tid; e0 < total; e0 += kBlock * RUN) {
#pragma unroll
                    for (int u = 0; u < RUN; ++u) {
                        const int e = e0 + kBlock * u, d = e & (RBD - 1), gx = xlo + (e >> 5);
                        const bool ok = e < total && d < nd && gx >= 0 && gx < NX;
                        const int idx = ok ? (db + d) * sd + gx * sx : 0;
                        SP_DCHECK(idx >= 0 && idx < plane);
                        xv[u] = ok ? ip[idx] : 0.f;
                        ev[u] = (MODE == RADON_RESIDUAL && ok) ? ep[idx] : 0.f;
                    }
#pragma unroll
                    for (int u = 0; u < RUN; ++u) {
                        const int e = e0 + kBlock * u;
                        if (e < total) {
                            SP_DCHECK((e >> 5) * RPI + (e & (RBD - 1)) < RXC * RPI);
                            L[(e >> 5) * RPI + (e & (RBD - 1))] = radon_x0v<MODE>(xv[u], ev[u], a, k);
                        }
                    }
                }
            }
            __syncthreads();
            if (active) {
                // RST steps' LDS reads are issued before the first is summed (the sum stays in
                // the order of d); a step past the band reads slab row d = nd - 1 again, unused
                for (int dq = 0; dq < nd; dq += RST) {
                    float w0[RST], f[RST], v0[RST], v1[RST];
#pragma unroll
                    for (int u = 0; u < RST; ++u) {
                        const int d = min(dq + u, nd - 1);
                        const int ic = radon_weights(
                            radon_pos(alpha, beta, ds, static_cast<float>(db + d) - d0, off), w0[u], f[u]);
                        SP_DCHECK(ic - xlo >= 0 && ic - xlo + 1 < XCn);
                        const int xc = min(max(ic - xlo, 0), XCn - 2);  // in the slab whatever the table
                        v0[u] = L[xc * RPI + d], v1[u] = L[(xc + 1) * RPI + d];
                    }
#pragma unroll
                    for (int u = 0; u < RST; ++u)
                        if (dq + u < nd) acc = radon_step(acc, w0[u], v0[u], f[u], v1[u]);
                }
            }
        } else if (active) {  // a slab too wide to stage: gather from global memory
            for (int d = 0; d < nd; ++d) {
                float w0, f;
                const int ic = radon_weights(
                    radon_pos(alpha, beta, ds, static_cast<float>(db + d) - d0, off), w0, f);
                float v0 = 0.f, v1 = 0.f;
                if (ic >= 0 && ic < NX) {
                    SP_DCHECK((db + d) * sd + ic * sx >= 0 && (db + d) * sd + ic * sx < plane);
                    v0 = radon_x0<MODE>(ip, ep, (db + d) * sd + ic * sx, a, k);
                }
                if (ic + 1 >= 0 && ic + 1 < NX) {
                    SP_DCHECK((db + d) * sd + (ic + 1) * sx >= 0 && (db + d) * sd + (ic + 1) * sx < plane);
                    v1 = radon_x0<MODE>(ip, ep, (db + d) * sd + (ic + 1) * sx, a, k);
                }
                acc = radon_step(acc, w0, v0, f, v1);
            }
        }
    }

    const int yplane = nA * D;  // <= 2^19
    const int q = ang * D + s;
    const float val = __fmul_rn(length, acc);
    float racc = 0.f;
    if (active) {
        SP_DCHECK(q >= 0 && q < yplane);
        float* __restrict__ op_out = out + (b * C + c) * static_cast<int64_t>(yplane);
        if constexpr (MODE == RADON_RESIDUAL) {
            const float r = y[((b / y_div) * C + c) * static_cast<int64_t>(yplane) + q] - val;
            op_out[q] = gs * r;
            racc = r * r;
        } else {
            op_out[q] = val;
        }
    }
    if constexpr (MODE == RADON_RESIDUAL) {
        const float t = block_sum(racc, red);
        SP_DCHECK(static_cast<int>(blockIdx.x) < P);
        if (tid == 0) partial[b * P + blockIdx.x] = t;
    }
}

// ray s of angle a on the pixel whose cross index is `target`: weight * g[a][s], or +0 when the
// ray is off the detector or does not touch the pixel (the load is made in bounds either way)
__device__ __forceinline__ float radon_term(const float* __restrict__ gp, int a, int D, int s,
                                            float alpha, float beta, float s0, float dd, float off,
                                            int target, int yplane) {
    float w0, f;
    const int ic = radon_weights(radon_pos(alpha, beta, static_cast<float>(s) - s0, dd, off), w0, f);
    const int sc = min(max(s, 0), D - 1);
    SP_DCHECK(a * D + sc >= 0 && a * D + sc < yplane);
    const float gv = gp[a * D + sc];
    const bool hit = s == sc && (ic == target || ic + 1 == target);
    return hit ? radon_mul(ic == target ? w0 : f, gv) : 0.f;
}

__global__ __launch_bounds__(kBlock) void k_radon_backproject(sp_op op, const float* __restrict__ g,
                                                              float* __restrict__ out, int tiles) {
    const int H = op.height, W = op.width, C = op.channels, nA = op.radius, D = op.factor;
    const int c = static_cast<int>(blockIdx.x) / tiles;
    const int tile = static_cast<int>(blockIdx.x) - c * tiles;
    const int64_t b = blockIdx.y;
    const int plane = H * W, yplane = nA * D;
    const int p = tile * kBlock + static_cast<int>(threadIdx.x);
    SP_DCHECK(c < C && tile * kBlock < plane);
    if (p >= plane) return;
    const int i = p / W, j = p - i * W;
    const float* __restrict__ gp = g + (b * C + c) * static_cast<int64_t>(yplane);
    const float s0 = 0.5f * static_cast<float>(D - 1);
    const float i0 = 0.5f * static_cast<float>(H - 1), j0 = 0.5f * static_cast<float>(W - 1);
    const float di = static_cast<float>(i) - i0, dj = static_cast<float>(j) - j0;

    float acc = 0.f;
    for (int a = 0; a < nA; ++a) {
        const float* __restrict__ row = op.taps + 4 * a;  // uniform: scalar loads
        const float alpha = row[0], beta = row[1], length = row[2];
        const bool axis = row[3] != 0.f;
        const float dd = axis ? dj : di, dx = axis ? di : dj, off = axis ? i0 : j0;
        const int target = axis ? i : j;
        // the locator only: the hardware reciprocal (1 ulp) moves it by < 1e-4
        const float sstar = s0 + (dx - beta * dd) * __builtin_amdgcn_rcpf(alpha);
        const int base = radon_floor(sstar) - 1;
        // a ray with a weight has |s - s*| < 1 + 1e-3 (file comment): base and base + 3 can be
        // one only when s* is that close to an integer; 1/64 leaves a wide margin
        const float fs = sstar - floorf(sstar);
        const bool lo = fs < 0.015625f, hi = fs > 0.984375f;
        // three evaluations without a branch (their loads in flight together): the inner two
        // and the one outer candidate that can count; summed in ascending s, absent terms as +0
        const float te = radon_term(gp, a, D, lo ? base : base + 3, alpha, beta, s0, dd, off, target, yplane);
        const float t1 = radon_term(gp, a, D, base + 1, alpha, beta, s0, dd, off, target, yplane);
        const float t2 = radon_term(gp, a, D, base + 2, alpha, beta, s0, dd, off, target, yplane);
        float t = __fadd_rn(lo ? te : 0.f, t1);
        t = __fadd_rn(__fadd_rn(t, t2), hi ? te : 0.f);
        acc = __fadd_rn(acc, radon_mul(length, t));
    }
    SP_DCHECK(p >= 0 && p < plane);
    out[(b * C + c) * static_cast<int64_t>(plane) + p] = acc;
}

// ---------------------------------------------------------------------------
// host side (called from the entry points in sp_dps.hip; `op` is valid)
// ---------------------------------------------------------------------------
bool radon_valid(const sp_op* op) {
    return op->taps && !op->keep_bits && !op->word_rank && op->radius >= 1 && op->radius <= 512 &&
           op->factor >= 1 && op->factor <= 1024 && op->channels > 0 && op->height >= 8 &&
           op->height <= 512 && op->width >= 8 && op->width <= 512 &&
           (int64_t)op->channels * op->height * op->width == op->n &&
           (int64_t)op->channels * op->radius * op->factor == op->m;
}

// ray chunks per angle: the fewest of <= kBlock rays, evenly sized
static inline int radon_chunks(const sp_op* op) { return (op->factor + kBlock - 1) / kBlock; }
static inline int radon_rays(const sp_op* op) {
    const int ch = radon_chunks(op);
    return (op->factor + ch - 1) / ch;
}

// workgroups per sample of `project` = r^2 partials per sample
int64_t radon_partials(const sp_op* op) { return (int64_t)op->channels * op->radius * radon_chunks(op); }

// floats of grad_scale * r between the project and the backproject launch
int64_t radon_workspace(const sp_op* op, int64_t batch) { return batch * op->m; }

static int radon_backproject(int kind, const char* what, const sp_op* op, const float* g, float* out,
                             int64_t batch, hipStream_t s) {
    const int tiles = (op->height * op->width + kBlock - 1) / kBlock;
    launch_w(kind, 0.0, k_radon_backproject, sample_grid((int64_t)op->channels * tiles, batch),
             dim3(kBlock), s, *op, g, out, tiles);
    return check_launch(what);
}

int radon_apply(const sp_op* op, const float* x, float* y, int64_t batch, hipStream_t s) {
    const int64_t P = radon_partials(op);
    launch_w(0, 0.0, k_radon_project<RADON_APPLY>, sample_grid(P, batch), dim3(kBlock), s, *op, x,
             (const float*)nullptr, (const float*)nullptr, (int64_t)1, 1.f, 0.f, 0.f, y,
             (float*)nullptr, static_cast<int>(P), radon_chunks(op), radon_rays(op),
             (const sp_step_rec*)nullptr, (const int32_t*)nullptr);
    return check_launch("sp_op_apply");
}

int radon_adjoint(const sp_op* op, const float* y, float* x, int64_t batch, hipStream_t s) {
    return radon_backproject(0, "sp_op_adjoint", op, y, x, batch, s);
}

// project (x, eps, y -> work = grad_scale r, partials), then backproject (work -> v)
int radon_dps_residual(const sp_op* op, const dps_residual_args& r, hipStream_t s) {
    const int64_t P = radon_partials(op);
    launch_w(TK_DPS_RESIDUAL, (double)r.batch, k_radon_project<RADON_RESIDUAL>, sample_grid(P, r.batch),
             dim3(kBlock), s, *op, r.x, r.eps, r.y, r.y_div, r.a, r.k, r.gs, r.work, r.partial,
             static_cast<int>(P), radon_chunks(op), radon_rays(op), r.sched, r.cursor);
    const int rc = check_launch("sp_dps_residual_ws");
    if (rc != SP_OK) return rc;
    return radon_backproject(TK_DPS_RESIDUAL, "sp_dps_residual_ws", op, r.work, r.v, r.batch, s);
}

}  // namespace sp
