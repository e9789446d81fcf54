"""Operands on which a correct fp32 kernel has no freedom, fp64 references for them, and plain
fp32 emulations of the kernels' algorithms on the CPU.

Integer convolution cases: x, w, bias, residual and dy hold integers of a range chosen from the
contraction length K so that 9 K max|x| max|w| 4 < 2^24.  Every product, every partial sum in
any order, and every intermediate of the F(2x2,3x3) Winograd algebra (multiples of 1/4: G's
halves) is then exactly representable in fp32, so a correct kernel returns the fp64 convolution
bit for bit: direct or Winograd, any k-step order, split-K and atomics included.

Dyadic GEMM cases: the bf16x6 GEMM (csrc/sp_gemm_x6.hip) splits each fp32 operand v into
h = the top 16 bits of v, m = the top 16 bits of v - h, l = the top 16 bits of v - h - m (exact:
3 x 8 significant bits), and keeps the products w_l x_h, w_h x_l, w_m x_m, w_m x_h, w_h x_m and
w_h x_h; it drops w_m x_l, w_l x_m and w_l x_l.  The classes here make every dropped product
zero and keep sum_k |w||x| + |bias| + |res| below 2^24 quanta (quantum = the product of the
operands' units), so every partial sum in every order is representable:
  a  x = k 2^-8, |k| < 2^11 (x_m live, x_l = 0), w in -3..3 (w_m = w_l = 0), dense
  b  the mirror image: w = k 2^-8, |k| < 2^11, x in -3..3
  c  x = k 2^-12, |k| < 2^20 (x_l live), w in {0, +-1, +-2} with sum |w| <= 8 per row of W
     (a dense row would need K |x| < 2^24: K = 16 at 20 bits leaves no room for a bias)
  d  x = k 2^-5 and w = k 2^-5, |k| < 2^10 (w_m x_m live; both l = 0), at most 8 non-zeros per
     row of W (10 + 10 bits of product leave 2^4 for the sum)
The non-zeros of c and d are spread over the whole row, so every k-step carries some.

Real-valued cases (``field``): randn, 30 + randn, and channels scaled by 2^+-12 alternately; for
them the yardstick of the per-output error rho = |y - y64| / (2^-24 E) is the emulation's own rho,
E being the envelope of the algorithm (direct: conv(|x|, |w|) + |bias| + |res|; Winograd: the same
algebra on absolute values).
"""

from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
FIELDS = ("randn", "offset30", "scaled")
GUARD_BITS = 0x5A5AA5A5  # the guard bands' fill (a finite float: 1.5389e16)


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def int_bound(k: int) -> int:
    """The largest r <= 4 with 9 k r r 4 < 2^24."""
    for r in (4, 3, 2, 1):
        if 9 * k * r * r * 4 < 2 ** 24:
            return r
    raise ValueError(k)


# --- convolution cases -----------------------------------------------------------------------


@dataclass
class ConvCase:
    """kind "s1": 3x3 / stride 1 / pad 1 on [n][cin][h][w]; "s2": 3x3 / stride 2 on x padded by one
    zero row / column bottom / right, y [h/2][w/2]; "up": stride 1 on the nearest-2x upsample of
    x [h/2][w/2], y [h][w].  y64 includes bias and res; dx64 is the input VJP of dy."""
    kind: str
    shape: tuple
    x: torch.Tensor
    w: torch.Tensor
    bias: torch.Tensor
    res: torch.Tensor
    dy: torch.Tensor
    y64: torch.Tensor
    dx64: torch.Tensor
    exact: bool

    @property
    def wt(self):
        """The input VJP's weights as a forward convolution's: transposed and flipped."""
        return self.w.transpose(0, 1).flip(2, 3).contiguous()


def conv_sizes(kind, shape):
    n, cin, cout, h, w = shape
    if kind == "s2":
        return (n, cin, h, w), (n, cout, h // 2, w // 2)
    if kind == "up":
        return (n, cin, h // 2, w // 2), (n, cout, h, w)
    return (n, cin, h, w), (n, cout, h, w)


def conv64(kind, x, w, bias):
    if kind == "s2":
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, bias, stride=2)
    if kind == "up":
        return F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, bias, padding=1)
    return F.conv2d(x, w, bias, padding=1)


def _finish(kind, shape, x, w, bias, res, dy, exact):
    if kind != "s1":  # the stride-2 and fused-upsample kernels take no residual
        res = torch.zeros_like(res)
    xd = x.double().requires_grad_()
    y = conv64(kind, xd, w.double(), bias.double())
    (dx,) = torch.autograd.grad(y, xd, dy.double())
    if kind == "s1":  # the issue's reference for the stride-1 VJP
        assert torch.equal(dx, torch.nn.grad.conv2d_input(x.shape, w.double(), dy.double(), padding=1))
    return ConvCase(kind, tuple(shape), x, w, bias, res, dy, y.detach() + res.double(), dx, exact)


def int_conv_case(shape, seed=0, kind="s1"):
    n, cin, cout, h, w = shape
    r = int_bound(max(cin, cout))
    g = gen(seed + 7 * sum(shape))
    xs, ys = conv_sizes(kind, shape)
    ri = lambda *s: torch.randint(-r, r + 1, s, generator=g).float()  # noqa: E731
    return _finish(kind, shape, ri(*xs), ri(cout, cin, 3, 3), ri(cout), ri(*ys), ri(*ys), True)


def real_conv_case(shape, field, seed=0, kind="s1"):
    n, cin, cout, h, w = shape
    g = gen(seed + 11 * sum(shape) + FIELDS.index(field))
    xs, ys = conv_sizes(kind, shape)
    x, dy = torch.randn(*xs, generator=g), torch.randn(*ys, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5
    if field == "offset30":
        x, dy = x + 30, dy + 30
    elif field == "scaled":  # channel c of x (and of dy) by 2^12 or 2^-12, alternately
        sc = lambda c: (2.0 ** (12 * (1 - 2 * (torch.arange(c) % 2)))).view(1, c, 1, 1)  # noqa: E731
        x, dy = x * sc(xs[1]), dy * sc(ys[1])
    return _finish(kind, shape, x, wt, torch.randn(cout, generator=g), torch.randn(*ys, generator=g), dy, False)


def impulse_conv_case(shape, seed=0, kind="s1"):
    """Unit impulses, each in a channel of its own (cyclically) and shifted by 5 channels per image,
    at the corners, the edge midpoints and both sides of every workgroup / wave seam (rows 7 | 8 and
    15 | 16, columns 15 | 16, 31 | 32 and 63 | 64; at 8 x 8 the image's last row and column are the
    seam to the next image of the mosaic; at stride 2 they lie next to the zero pad), bias and
    residual 0, integer weights."""
    n, cin, cout, h, w = shape
    g = gen(seed + 13 * sum(shape))
    xs, ys = conv_sizes(kind, shape)
    hx, wx = xs[2], xs[3]
    rows = sorted({0, hx // 2, hx - 1} | {r for r in (7, 8, 15, 16) if r < hx})
    cols = sorted({0, wx // 2, wx - 1} | {c for c in (15, 16, 31, 32, 63, 64) if c < wx})
    x = torch.zeros(*xs)
    k = 0
    if (hx, wx) == (8, 8):  # the mosaic: the last row / column of even images, the first of odd ones
        for s in range(n):
            for k, (i, j) in enumerate(((7, 7), (7, 4), (4, 7)) if s % 2 == 0 else ((0, 0), (0, 4), (4, 0))):
                x[s, (k + 5 * s) % cin, i, j] = 1.0
        rows = cols = []
    for i in rows:
        for j in cols:
            if i in (0, hx - 1, 7, 8, 15, 16) or j in (0, wx - 1, 15, 16, 31, 32, 63, 64):
                for s in range(n):
                    x[s, (k + 5 * s) % cin, i, j] = 1.0
                k += 1
    wt = torch.randint(-4, 5, (cout, cin, 3, 3), generator=g).float()
    dy = torch.randint(-4, 5, ys, generator=g).float()
    return _finish(kind, shape, x, wt, torch.zeros(cout), torch.zeros(*ys), dy, True)


# --- fp32 emulations of the convolution algorithms -------------------------------------------


def emu_direct(x, w, bias=None, res=None, reverse=False, dtype=F32, absolute=False):
    """3x3 / pad 1 convolution accumulated sequentially over (ci, tap) in ``dtype``, forward or in
    reversed order, then + bias, + res.  absolute: on absolute values (the direct envelope)."""
    x, w = x.to(dtype), w.to(dtype)
    if absolute:
        x, w, bias, res = x.abs(), w.abs(), None if bias is None else bias.abs(), None if res is None else res.abs()
    n, cin, h, wd = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    acc = torch.zeros(n, w.shape[0], h, wd, dtype=dtype)
    order = [(ci, t) for ci in range(cin) for t in range(9)]
    for ci, t in (reversed(order) if reverse else order):
        ky, kx = divmod(t, 3)
        acc += w[:, ci, ky, kx].view(1, -1, 1, 1) * xp[:, ci, ky:ky + h, kx:kx + wd].unsqueeze(1)
    if bias is not None:
        acc = acc + bias.to(dtype).view(1, -1, 1, 1)
    return acc if res is None else acc + res.to(dtype)


def _bt(d, dim, s):  # rows of B^T d: d0 - d2, d1 + d2, d2 - d1, d1 - d3 (s = -1: on absolute values)
    d0, d1, d2, d3 = d.unbind(dim)
    return torch.stack((d0 - s * d2, d1 + d2, d2 - s * d1, d1 - s * d3), dim)


def _g(g, dim, s):  # rows of G g, G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]] (wino_filter's order)
    g0, g1, g2 = g.unbind(dim)
    return torch.stack((g0, 0.5 * (g0 + g1 + g2), 0.5 * (g0 - s * g1 + g2), g2), dim)


def _at(m, dim, s):  # rows of A^T m: m0 + m1 + m2, m1 - m2 - m3
    m0, m1, m2, m3 = m.unbind(dim)
    return torch.stack((m0 + m1 + m2, m1 - s * m2 - s * m3), dim)


def emu_wino(x, w, bias=None, res=None, dtype=F32, absolute=False):
    """F(2x2,3x3): U = G g G^T, V = B^T d B, M = sum over ci of U V accumulated sequentially in
    ``dtype``, Y = A^T M A, then + bias, + res.  absolute: the same algebra on absolute values
    (|A^T| [(|G||w||G^T|) (|B^T||d||B|)] |A|): the Winograd envelope."""
    s = -1.0 if absolute else 1.0
    x, w = x.to(dtype), w.to(dtype)
    if absolute:
        x, w = x.abs(), w.abs()
    n, cin, h, wd = x.shape
    cout = w.shape[0]
    u = _g(_g(w, 2, s), 3, s)                                            # [co][ci][4][4]
    d = F.pad(x, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)           # [n][ci][th][tw][4][4]
    v = _bt(_bt(d, 4, s), 5, s)
    m = torch.zeros(n, cout, h // 2, wd // 2, 4, 4, dtype=dtype)
    for ci in range(cin):
        m += u[:, ci].view(1, cout, 1, 1, 4, 4) * v[:, ci].unsqueeze(1)
    y = _at(_at(m, 4, s), 5, s)                                          # [n][co][th][tw][2][2]
    y = y.permute(0, 1, 2, 4, 3, 5).reshape(n, cout, h, wd)
    if bias is not None:
        y = y + (bias.abs() if absolute else bias).to(dtype).view(1, -1, 1, 1)
    if res is not None:
        y = y + (res.abs() if absolute else res).to(dtype)
    return y


def _up(x):
    return F.interpolate(x, scale_factor=2.0, mode="nearest")


def _odd(z):
    return z[..., 1::2, 1::2]


def _stuff(dy):  # the stride-2 VJP's dy at the odd positions of the full-resolution grid
    z = torch.zeros(dy.shape[0], dy.shape[1], 2 * dy.shape[2], 2 * dy.shape[3], dtype=dy.dtype)
    z[..., 1::2, 1::2] = dy
    return z


def _pool(z):  # 2x2 block sums in sp_upsample2x_vjp's order: (a + b) + (c + d) per block
    return (z[..., 0::2, 0::2] + z[..., 0::2, 1::2]) + (z[..., 1::2, 0::2] + z[..., 1::2, 1::2])


def emu_forward(case: ConvCase, algo, **kw):
    """y of ``case`` by emulation ``algo`` (emu_direct or emu_wino); the stride-2 convolution is the
    stride-1 one read at the odd positions, the fused upsample the stride-1 one on the upsample."""
    if case.kind == "s2":
        y = _odd(algo(case.x, case.w, **kw))
        b = case.bias.to(y.dtype).view(1, -1, 1, 1)
        return y + (b.abs() if kw.get("absolute") else b)
    x = _up(case.x) if case.kind == "up" else case.x
    return algo(x, case.w, case.bias, case.res, **kw)


def emu_vjp(case: ConvCase, algo, **kw):
    if case.kind == "s2":
        return algo(_stuff(case.dy), case.wt, **kw)
    dx = algo(case.dy, case.wt, **kw)
    return _pool(dx) if case.kind == "up" else dx


def rho(got, want, env):
    """max over outputs of |got - want| / (2^-24 env) (outputs with a zero envelope must be exact)."""
    err = (got.double() - want).abs()
    env = env.double()
    assert bool((err[env == 0] == 0).all())
    return float((err / (2.0 ** -24 * env).clamp_min(1e-300)).max())


def rel_l2(got, want):
    return float((got.double() - want).norm() / want.norm())


# --- dyadic GEMM cases for the bf16x6 split ---------------------------------------------------


def g6_split(v):
    """(h, m, l) of csrc/sp_gemm_x6.hip's g6_split on an fp32 tensor: bit-mask truncations."""
    v = v.contiguous()
    top = lambda t: (t.view(torch.int32) & -65536).view(F32)  # noqa: E731
    h = top(v)
    r = v - h
    m = top(r)
    return h, m, top(r - m)


KEPT = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1))  # (W term, X term) of the small accumulator, in order


def emu_x6(W, X, bias=None, res=None):
    """Y [m][cols] = W [m][k] X [k][cols] as k_gemm_x6 computes it: per k-step of 16 the five small
    products into one fp32 accumulator and w_h x_h into another, y = (acc + acs) + bias + res."""
    wt, xt = g6_split(W), g6_split(X)
    acc = torch.zeros(W.shape[0], X.shape[1])
    acs = torch.zeros_like(acc)
    for s in range(0, W.shape[1], 16):
        for tu, tv in KEPT:
            acs += wt[tu][:, s:s + 16] @ xt[tv][s:s + 16]
        acc += wt[0][:, s:s + 16] @ xt[0][s:s + 16]
    y = acc + acs
    if bias is not None:
        y = y + bias.view(-1, 1)
    return y if res is None else y + res


@dataclass
class GemmCase:
    """Y [m][cols] = W [m][k] X [k][cols] + bias[:, None] + res; quantum: the unit of every product."""
    cls: str
    W: torch.Tensor
    X: torch.Tensor
    bias: torch.Tensor
    res: torch.Tensor
    y64: torch.Tensor
    quantum: float

    @property
    def env(self):
        return self.W.double().abs() @ self.X.double().abs() + self.bias.double().abs().view(-1, 1) + \
            self.res.double().abs()


def _sparse_rows(m, k, nnz, draw, g):
    """[m][k] with nnz non-zeros per row at distinct random columns (every k-step gets some)."""
    W = torch.zeros(m, k)
    cols = torch.rand(m, k, generator=g).argsort(1)[:, :min(nnz, k)]
    W.scatter_(1, cols, draw(m, cols.shape[1]))
    return W


def dyadic_gemm_case(cls, m, k, cols, seed=0):
    g = gen(seed + 17 * (m + k + cols) + ord(cls))
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()  # noqa: E731
    nz = lambda hi, *s: ri(1, hi, *s) * (2 * ri(0, 1, *s) - 1)  # noqa: E731  (non-zero, either sign)
    if cls == "a":
        W, X, q = ri(-3, 3, m, k), ri(-2047, 2047, k, cols) * 2.0 ** -8, 2.0 ** -8
    elif cls == "b":
        W, X, q = ri(-2047, 2047, m, k) * 2.0 ** -8, ri(-3, 3, k, cols), 2.0 ** -8
    elif cls == "c":
        W = _sparse_rows(m, k, 4, lambda *s: nz(2, *s), g)
        X, q = ri(-2 ** 20 + 1, 2 ** 20 - 1, k, cols) * 2.0 ** -12, 2.0 ** -12
    elif cls == "d":
        W = _sparse_rows(m, k, 8, lambda *s: nz(1023, *s) * 2.0 ** -5, g)
        X, q = ri(-1023, 1023, k, cols) * 2.0 ** -5, 2.0 ** -10
    else:
        raise ValueError(cls)
    bias = ri(-64, 64, m) * (q * 256)
    res = ri(-64, 64, m, cols) * (q * 256)
    y64 = W.double() @ X.double() + bias.double().view(-1, 1) + res.double()
    return GemmCase(cls, W, X, bias, res, y64, q)


def real_gemm_case(field, m, k, cols, seed=0):
    g = gen(seed + 19 * (m + k + cols) + FIELDS.index(field))
    W = torch.randn(m, k, generator=g) * k ** -0.5
    X = torch.randn(k, cols, generator=g)
    if field == "offset30":
        X = X + 30
    elif field == "scaled":
        X = X * (2.0 ** (12 * (1 - 2 * (torch.arange(k) % 2)))).view(k, 1)
    bias, res = torch.randn(m, generator=g), torch.randn(m, cols, generator=g)
    y64 = W.double() @ X.double() + bias.double().view(-1, 1) + res.double()
    return GemmCase(field, W, X, bias, res, y64, 0.0)


# --- sentinel buffers for the GPU tests -----------------------------------------------------


class Guarded:
    """A NaN-filled tensor of ``shape`` inside a larger buffer whose bands before and after it
    (``guard`` floats each, rounded up to 256 B) hold GUARD_BITS."""

    def __init__(self, shape, guard, device, fill=float("nan")):
        numel = 1
        for s in shape:
            numel *= s
        self.g = (max(guard, 64) + 63) // 64 * 64
        self.buf = torch.full((2 * self.g + numel,), GUARD_BITS, dtype=torch.int32, device=device).view(F32)
        self.t = self.buf[self.g:self.g + numel].view(*shape)
        self.t.fill_(fill)

    def ptr(self):
        return self.t.data_ptr()

    def check(self, nan_ok=False):
        """The tensor, after asserting that the bands are untouched and (an output) no NaN is left."""
        band = self.buf.view(torch.int32)
        assert bool((band[:self.g] == GUARD_BITS).all()), "the guard band before the buffer was written"
        assert bool((band[band.numel() - self.g:] == GUARD_BITS).all()), "the guard band after the buffer was written"
        if not nan_ok:
            assert not bool(torch.isnan(self.t).any()), f"{int(torch.isnan(self.t).sum())} outputs never written"
        return self.t


def assert_bitwise(got, want64, what=""):
    """got (fp32) equals the fp64 reference, itself an fp32 number, in every element; on a mismatch the
    count and the first coordinates (the tile, wave and k-step to read the kernel at)."""
    got, want = got.detach().cpu(), want64.float()
    assert torch.equal(want.double(), want64.double()), "the reference is not an fp32 number"
    assert got.shape == want.shape, (got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        first = [(tuple(i.tolist()), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:6]]
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} outputs differ; (index, got, want): {first}")


# --- the shapes (n, cin, cout, h, w) the CPU and GPU tests share ----------------------------

WINO_W32 = [(3, 16, 64, 8, 32), (2, 24, 128, 24, 64), (1, 40, 64, 16, 96)]
WINO_W16 = [(3, 16, 64, 16, 16), (2, 24, 128, 48, 16)]
WINO_MOSAIC = [(n, 16, 64, 8, 8) for n in (1, 2, 3, 4, 5, 7)] + [(5, 24, 128, 8, 8)]
WINO_SPLIT = [(1, 32, 64, 8, 8), (1, 64, 64, 16, 16), (1, 96, 64, 8, 32), (1, 128, 64, 8, 32), (1, 256, 64, 8, 8),
              (1, 512, 64, 16, 16), (1, 1024, 64, 8, 32)]
WINO_UP = [(1, 64, 64, 32, 32), (1, 128, 128, 32, 64)]
DIRECT = [(2, 4, 128, 8, 32), (1, 12, 256, 16, 64), (3, 132, 128, 8, 96)]
S2_FWD = [(1, 4, 128, 16, 64), (2, 12, 256, 32, 64), (1, 32, 128, 16, 64)]   # the last one splits K in two
S2_VJP = [(1, 128, 4, 4, 64), (2, 256, 8, 8, 128), (1, 128, 32, 4, 64)]
THIN = [(1, 1, 1, 1, 4), (2, 3, 5, 9, 68), (1, 8, 8, 7, 12), (2, 200, 8, 8, 72), (2, 8, 200, 8, 72)]
IMPULSE = [("s1", (1, 40, 64, 16, 96)), ("s1", (2, 24, 128, 24, 64)), ("s1", (2, 24, 128, 48, 16)),
           ("s1", (5, 24, 128, 8, 8)), ("s1", (7, 16, 64, 8, 8)), ("s1", (3, 132, 128, 8, 96)),
           ("s2", (2, 12, 256, 32, 64)), ("s1", (2, 3, 5, 9, 68)), ("up", (1, 64, 64, 32, 32))]


def swapped(shape):
    """The layer whose input VJP contracts over ``shape``'s cin and produces its cout channels."""
    n, cin, cout, h, w = shape
    return (n, cout, cin, h, w)


GEMM_K = (16, 32, 80, 96, 112, 208)  # k-steps: 1, 2 (< the 6-slot ring), ring - 1, ring, ring + 1, two wraps
GEMM_CLASSES = "abcd"


# Relative L2 (forward, input VJP) of emu_wino against fp64 on the operands of tests/test_conv_gpu.py's raw
# Winograd tests (test_winograd_forward_and_input_vjp: seed 11 + sum(shape), forward with bias;
# test_winograd_split_k_workspace: seed 41 + sum(shape), forward with bias and residual), computed once on the
# CPU; those tests bound the tile by twice these.  tests/test_exact_cases.py recomputes the cheap ones.
WINO_EMU_L2 = {
    "raw": {
        (2, 128, 128, 32, 64): (2.54e-07, 3.60e-07), (1, 256, 64, 16, 32): (3.75e-07, 2.70e-07),
        (2, 64, 128, 8, 96): (1.84e-07, 3.66e-07), (3, 64, 192, 24, 64): (1.92e-07, 4.34e-07),
        (3, 128, 64, 16, 16): (2.61e-07, 2.75e-07), (2, 64, 128, 32, 16): (1.98e-07, 3.66e-07),
        (1, 512, 512, 16, 16): (4.84e-07, 6.98e-07), (3, 64, 128, 8, 8): (2.03e-07, 3.71e-07),
        (5, 512, 512, 8, 8): (4.77e-07, 7.08e-07), (8, 128, 64, 8, 8): (2.66e-07, 2.79e-07),
        (64, 512, 512, 8, 8): (4.99e-07, 7.12e-07), (12, 256, 128, 8, 8): (3.41e-07, 3.72e-07),
        (2, 24, 64, 8, 32): (1.35e-07, 2.77e-07), (2, 32, 64, 16, 64): (1.49e-07, 2.72e-07),
        (1, 48, 64, 8, 32): (1.59e-07, 2.74e-07),
    },
    "split": {
        (1, 128, 128, 128, 128): (2.08e-07, 3.59e-07), (1, 256, 256, 64, 64): (2.88e-07, 4.95e-07),
        (1, 512, 512, 32, 32): (3.94e-07, 6.95e-07), (1, 512, 512, 16, 16): (3.96e-07, 6.97e-07),
        (1, 512, 512, 8, 8): (3.94e-07, 7.08e-07), (3, 256, 128, 8, 8): (2.79e-07, 3.70e-07),
        (2, 64, 128, 32, 64): (1.61e-07, 3.58e-07),
    },
}


def raw_wino_operands(shape, split):
    """(x, w, bias, res or None, dy) as the two raw Winograd tests of tests/test_conv_gpu.py draw them."""
    n, cin, cout, h, w = shape
    g = gen((41 if split else 11) + sum(shape))
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (cin * 9) ** -0.5
    b = torch.randn(cout, generator=g)
    res = torch.randn(n, cout, h, w, generator=g) if split else None
    return x, wt, b, res, torch.randn(n, cout, h, w, generator=g)
