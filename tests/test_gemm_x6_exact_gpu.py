"""The bf16x6 GEMM (csrc/sp_gemm_x6.hip) held to bit-exact dyadic cases, and per output on real data.

tests/test_gemm_x6_gpu.py bounds one relative-L2 number per tensor on randn data.  The kernel claims
exact three-term operand splits; tests/exact_cases.py builds operand classes a-d for which every
product it drops is zero and no partial sum can round (shown on the CPU by tests/test_exact_cases.py),
each exercising another term of the split (a, b: the second term of x / of W; c: the third term of x;
d: the second terms' product).  A correct kernel then returns the fp64 product bit for bit through
sp_gemm_x6, sp_linear_x6, sp_gemm_x6_layout and their split-K forms: ``torch.equal`` on NaN-filled
outputs between guard bands.

K in 16, 32, 80, 96, 112, 208: 1, 2, 5, 6, 7 and 13 k-steps against the 6-slot X ring (one step, fewer
than the ring, ring - 1, the ring, ring + 1, two wraps).  m = 32, 96, 160 on the token-major forms: the
last 128-row block of W is partly zero padding, whose rows must contribute nothing and store nothing.

The second half: rho = |y - y64| / (2^-24 (|W||x| + |bias| + |res|)) per output on randn, 30 + randn and
channels scaled by 2^+-12, against the emulation of the split and its six kept products (ec.emu_x6).
Measured on an MI355X: see README "Exact cases".
"""

from __future__ import annotations

import pytest
import torch

import exact_cases as ec
from samplers_amd import _hip
from test_gemm_x6_gpu import SPLIT_CASES

pytestmark = pytest.mark.gpu


class X6:
    def __init__(self, cuda):
        self.lib = _hip.load_library()
        self.cuda = cuda
        self.st = torch.cuda.current_stream().cuda_stream

    def dev(self, t):
        return None if t is None else t.to(self.cuda).contiguous()

    def pack(self, W, trans=0):
        m, k = W.shape
        wg = self.dev(W.t() if trans else W)  # trans: W stored [K][M]
        wp = torch.empty(int(self.lib.sp_gemm_x6_packed_size(m, k)), device=self.cuda)
        _hip.check(self.lib.sp_gemm_x6_pack(wg.data_ptr(), m, k, trans, wp.data_ptr(), self.st), "sp_gemm_x6_pack")
        return wp

    @staticmethod
    def img(t, n):  # [c][n hw] -> [n][c][hw]
        return t.view(t.shape[0], n, -1).permute(1, 0, 2).contiguous()

    def run(self, kind, c, n, bias=True, res=True, c1=None, o1=None, in_tm=0, out_tm=0, trans=0, split=False):
        """Y [m][n hw] of case c through ``kind`` (gemm / linear / layout); rows / columns as the case's."""
        lib, st, p = self.lib, self.st, _hip.ptr
        m, k = c.W.shape
        cols = c.X.shape[1]
        hw = cols // n
        wp = self.pack(c.W, trans)
        bg = self.dev(c.bias) if bias else None
        nb = int(lib.sp_gemm_x6_workspace(n if kind != "linear" else 1, hw if kind != "linear" else cols, k, m)) \
            if split else 0
        assert not split or nb > 0
        ws = ec.Guarded((max(nb // 4, 1),), hw, self.cuda)
        wsp = ws.ptr() if split else None
        if kind == "gemm":
            c1 = k if c1 is None else c1
            o1 = m if o1 is None else o1
            assert lib.sp_gemm_x6_supported(m, k, hw) and not (res and o1 < m)
            x1, x2 = self.dev(self.img(c.X[:c1], n)), self.dev(self.img(c.X[c1:], n)) if c1 < k else None
            rg = self.dev(self.img(c.res, n)) if res else None
            y1 = ec.Guarded((n, o1, hw), o1 * hw, self.cuda)
            y2 = ec.Guarded((n, m - o1, hw), (m - o1) * hw, self.cuda) if o1 < m else None
            _hip.check(lib.sp_gemm_x6_ws(p(x1), c1, p(x2), k - c1, p(wp), p(bg), p(rg), n, hw, y1.ptr(), o1,
                                         None if y2 is None else y2.ptr(), m - o1, wsp, nb, st), "sp_gemm_x6_ws")
            torch.cuda.synchronize()
            ws.check(nan_ok=True)
            y = y1.check() if y2 is None else torch.cat([y1.check(), y2.check()], 1)
            return y.permute(1, 0, 2).reshape(m, cols)
        if kind == "linear":
            in_tm = out_tm = 1
            assert lib.sp_linear_x6_supported(cols, k, m)
        else:
            assert lib.sp_gemm_x6_layout_supported(n, hw, k, m)
        xg = self.dev(c.X.t() if in_tm else self.img(c.X, n))
        rg = None if not res else self.dev(c.res.t() if out_tm else self.img(c.res, n))
        y = ec.Guarded((cols, m) if out_tm else (n, m, hw), 256 * m, self.cuda)
        if kind == "linear":
            _hip.check(lib.sp_linear_x6_ws(p(xg), p(wp), p(bg), p(rg), cols, k, m, y.ptr(), wsp, nb, st), "sp_linear_x6_ws")
        else:
            _hip.check(lib.sp_gemm_x6_layout_ws(p(xg), p(wp), p(bg), p(rg), n, hw, k, m, in_tm, out_tm, y.ptr(),
                                                wsp, nb, st), "sp_gemm_x6_layout_ws")
        torch.cuda.synchronize()
        ws.check(nan_ok=True)
        return y.check().t() if out_tm else y.check().permute(1, 0, 2).reshape(m, cols)


@pytest.fixture(scope="module")
def x6(cuda):
    return X6(cuda)


def _want(c, bias=True, res=True):
    y = c.y64
    if not bias:
        y = y - c.bias.double().view(-1, 1)
    return y if res else y - c.res.double()


@pytest.mark.parametrize("k", ec.GEMM_K)
@pytest.mark.parametrize("cls", ec.GEMM_CLASSES)
def test_gemm_x6_image_major_is_exact(x6, cls, k):
    """sp_gemm_x6 (k_gemm_x6<false, false>): m = 128 at hw = 256 over two images and m = 256 at hw = 768,
    with bias and residual and without; two inputs split at c1 = 16 and K - 16; two outputs split at
    o1 = 32 and m - 32 (no residual there)."""
    for m, hw, n in ((128, 256, 2), (256, 768, 1)):
        c = ec.dyadic_gemm_case(cls, m, k, n * hw)
        ec.assert_bitwise(x6.run("gemm", c, n), c.y64, f"sp_gemm_x6 {cls} m {m} k {k} hw {hw}")
        ec.assert_bitwise(x6.run("gemm", c, n, bias=False, res=False), _want(c, False, False),
                          f"sp_gemm_x6 plain {cls} m {m} k {k} hw {hw}")
        for c1 in sorted({16, k - 16} - {0}):
            ec.assert_bitwise(x6.run("gemm", c, n, c1=c1), c.y64, f"sp_gemm_x6 two inputs c1 {c1} {cls} m {m} k {k}")
        for o1 in (32, m - 32):
            ec.assert_bitwise(x6.run("gemm", c, n, res=False, o1=o1), _want(c, True, False),
                              f"sp_gemm_x6 two outputs o1 {o1} {cls} m {m} k {k}")


@pytest.mark.parametrize("k", ec.GEMM_K)
@pytest.mark.parametrize("cls", ec.GEMM_CLASSES)
def test_linear_and_layout_x6_are_exact(x6, cls, k):
    """sp_linear_x6 (k_gemm_x6<true, true>) and sp_gemm_x6_layout's four layout pairs (<in_tm, out_tm>) at
    m = 32, 96, 160: the last (only) 128-row block of W is partly padding."""
    for i, m in enumerate((32, 96, 160)):
        n, hw = ((1, 768), (3, 256), (1, 256))[i]
        c = ec.dyadic_gemm_case(cls, m, k, n * hw)
        extras = (i + k // 16) % 2 == 0
        want = _want(c, extras, extras)
        ec.assert_bitwise(x6.run("linear", c, 1, extras, extras), want, f"sp_linear_x6 {cls} m {m} k {k}")
        for in_tm in (0, 1):
            for out_tm in (0, 1):
                ec.assert_bitwise(x6.run("layout", c, n, not extras, not extras, in_tm=in_tm, out_tm=out_tm),
                                  _want(c, not extras, not extras),
                                  f"sp_gemm_x6_layout {in_tm}{out_tm} {cls} m {m} k {k} n {n}")


@pytest.mark.parametrize("cls", ec.GEMM_CLASSES)
def test_x6_transposed_pack_is_exact(x6, cls):
    """sp_gemm_x6_pack(trans = 1) from W stored [K][M]: the same packed fragments, the same bits out."""
    for kind, m, k, n, hw in (("gemm", 128, 112, 1, 256), ("linear", 96, 80, 1, 256)):
        c = ec.dyadic_gemm_case(cls, m, k, n * hw, seed=1)
        ec.assert_bitwise(x6.run(kind, c, n, trans=1), c.y64, f"{kind} trans {cls}")


@pytest.mark.parametrize("case", SPLIT_CASES)
@pytest.mark.parametrize("cls", ec.GEMM_CLASSES)
def test_x6_split_k_is_exact(x6, cls, case):
    """The split-K forms at tests/test_gemm_x6_gpu.py's SPLIT_CASES (K up to 768: 2-16 parts stored to a
    NaN-filled workspace and added by k_g6_split_reduce with the bias and the residual).  Class a and b
    stay below 2^24 quanta up to K = 2730; c and d bound each row of W, not K."""
    kind, n, hw, k, m, o2, in_tm, out_tm, extras = case
    c = ec.dyadic_gemm_case(cls, m, k, n * hw, seed=2)
    res = extras and not o2
    got = x6.run(kind, c, n, extras, res, o1=m - o2 if kind == "gemm" else None, in_tm=in_tm, out_tm=out_tm, split=True)
    ec.assert_bitwise(got, _want(c, extras, res), f"split {case} {cls}")


@pytest.mark.parametrize("a", [-40, 17, 60])
def test_x6_power_of_two_scaling_is_bitwise(x6, a):
    """W times 2^a and x times 2^-a on randn data: every term of both splits moves by a power of two, so
    every product and the output (bias and residual unscaled) keep their bits.  An exponent-dependent
    mistake in the split (a mask applied to the wrong field, a term flushed) would show here."""
    for kind, m, k, n, hw in (("gemm", 128, 208, 1, 256), ("linear", 96, 112, 1, 256)):
        c = ec.real_gemm_case("randn", m, k, n * hw)
        y0 = x6.run(kind, c, n)
        c.W, c.X = c.W * 2.0 ** a, c.X * 2.0 ** -a
        assert torch.equal(x6.run(kind, c, n), y0), (kind, a)


@pytest.mark.parametrize("field", ec.FIELDS)
@pytest.mark.parametrize("kind,m,k,n,hw,split", [("gemm", 128, 208, 2, 256, False), ("gemm", 256, 512, 1, 256, True),
                                                  ("linear", 96, 112, 1, 768, False), ("linear", 320, 512, 1, 256, True),
                                                  ("layout", 160, 80, 3, 256, False)])
def test_x6_every_output_within_the_emulations_error(x6, parity_record, kind, m, k, n, hw, split, field):
    """max rho(GPU) <= 4 max rho(emulation), relative L2 <= 2 x the emulation's (with bias and residual)."""
    c = ec.real_gemm_case(field, m, k, n * hw)
    got = x6.run(kind, c, n, in_tm=1 if kind == "layout" else 0, split=split).cpu()
    emu = ec.emu_x6(c.W, c.X, c.bias, c.res)
    r_gpu, r_emu = ec.rho(got, c.y64, c.env), ec.rho(emu, c.y64, c.env)
    l_gpu, l_emu = ec.rel_l2(got, c.y64), ec.rel_l2(emu, c.y64)
    parity_record(f"x6_{kind}_rho", r_gpu, 4 * r_emu, m=m, k=k, cols=n * hw, split=split, field=field, emulation=r_emu)
    parity_record(f"x6_{kind}_rel_l2", l_gpu, 2 * l_emu, m=m, k=k, cols=n * hw, split=split, field=field, emulation=l_emu)
    print(f"x6 {kind} m {m} k {k} {field}: rho {r_gpu:.3f} (emulation {r_emu:.3f}), rel L2 {l_gpu:.2e} ({l_emu:.2e})")
    assert r_gpu <= 4 * r_emu, (r_gpu, r_emu)
    assert l_gpu <= 2 * l_emu, (l_gpu, l_emu)
