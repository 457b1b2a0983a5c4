"""GPU leg: the GEMM family behind memory fences, every element against an fp64 bound (tests/gemm_check.py).

Every launch of this file runs with
  * A as a fenced view (lda = K + 64, NaN around it, NaN spare rows behind the rows the launch uses where `rows=` is passed),
  * W as a row slice of a NaN-fenced buffer, bias / gate / residual / blend / alpha / norm weights as fenced views,
  * the output as a fenced view at column offset 8 with ldc = nout + 16 (fp32 stream: offset 4, ldc32 = N + 8), the whole buffer -
    the view included - pre-filled with the sentinel NaN pattern,
and asserts after it: the output fence is bit-identical, the result holds no NaN / Inf (so every element was written, and no
fenced operand value reached a product), and max |got - ref| / bound <= 1 per element.  Which kernel family serves a launch follows
from the selection rule at dwm_gemm_args.tile (include/dwm_hip.h); for the 4-wave kernels it is asserted through the launch
counters.  One line per family with the worst ratio and its shape goes to the suite's parity log (`_log` of tests/test_hip_gpu.py).

M in {1, 255, 256, 257} x N in {8, 120, 128, 136, 248, 264} x K in {64, 128, 192}: all 24 (M, N) pairs, K = Ks[(i + j) % 3], which
covers every (M, K) and (N, K) pair as well."""
import pytest
import torch

from tests import gemm_check as G
from tests.test_hip_gpu import TOL_KERNEL, _log

pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32

MS, NS, KS = (1, 255, 256, 257), (8, 120, 128, 136, 248, 264), (64, 128, 192)
PAIRWISE = [(M, N, KS[(i + j) % 3]) for i, M in enumerate(MS) for j, N in enumerate(NS)]
ACTS = ("none", "gelu_tanh", "silu", "relu")
# the six operand sets of test_gemm_resid and the two in-place forms
RESID_FORMS = ("gate_res", "res_blend", "res", "mod_pos", "mod_neg", "mod_neg_relu", "gate_res_inplace", "res_blend_inplace")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def worst():
    """family -> (worst element ratio, where); one log line per family when the module is done"""
    d = {}
    yield d
    for fam, (ratio, where) in d.items():
        _log("gemm_fence", family=fam, worst_ratio=ratio, at=where)


def _note(worst, family, ratio, **where):
    if family not in worst or ratio > worst[family][0]:
        worst[family] = (ratio, where)


def _rand(shape, dev, seed, scale=1.0, dtype=bf16):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev).to(dtype)


def _act_code(act):
    from opendwm_amd import ops
    return {"none": ops.ACT_NONE, "gelu_tanh": ops.ACT_GELU_TANH, "silu": ops.ACT_SILU, "relu": ops.ACT_RELU}[act]


def _verify(view, buf, ref, K, tag):
    """the three assertions behind every launch; returns the ratio"""
    assert G.untouched(buf, view), ("output fence touched", tag)
    assert bool(torch.isfinite(view).all()), ("NaN / Inf in the result", tag, torch.nonzero(~torch.isfinite(view))[:20].tolist())
    ratio = G.check(view, ref, K)
    if not ratio <= 1:
        print("over the bound", tag, "(row, column, got, ref, ratio):")
        for line in G.worst(view, ref, K):
            print("   ", line)
    assert ratio <= 1, (ratio, tag)
    return ratio


class Problem:
    """one (M, N, K) with fenced A / W / bias and the fp64 products; `run` launches one epilogue form and checks it"""

    def __init__(self, dev, M, N, K, spare=0, a=None):
        self.dev, self.M, self.N, self.K, self.spare = dev, M, N, K, spare
        self.a, self.a_buf = G.fenced((M + spare, K), bf16, dev, col_off=16, pad_cols=48)
        G.put(self.a[:M], _rand((M, K), dev, 1) if a is None else a)
        self.w_plain = _rand((N, K), dev, 2, K ** -0.5)
        self.b_plain = _rand((N,), dev, 3)
        self.w, self.w_buf = G.fenced((N, K), bf16, dev, col_off=0, pad_cols=0)
        G.put(self.w, self.w_plain)
        self.b, self.b_buf = G.fenced_vec(N, bf16, dev)
        G.put(self.b, self.b_plain)
        self.prod = G.product(self.a[:M], self.w)
        self.rows_kw = dict(rows=M) if spare else {}
        self.gemm_kw = {}                   # a_grid / conv3x3 of the implicit convolution
        self._data = {}

    def data(self, name, shape, seed, dtype=bf16):
        key = (name, tuple(shape), dtype)
        if key not in self._data:
            if name == "alpha":
                self._data[key] = torch.rand(shape, generator=torch.Generator().manual_seed(seed)).to(self.dev)
            else:
                self._data[key] = _rand(shape, self.dev, seed, dtype=dtype)
        return self._data[key]

    def operand(self, name, shape, seed, dtype=bf16, fill=G.NAN):
        q = 8 if dtype == bf16 else 4
        view, buf = G.fenced(shape, dtype, self.dev, col_off=q, pad_cols=q, fill=fill)
        G.put(view, self.data(name, shape, seed, dtype))
        return view, buf

    def resid_operands(self, form, rpg, stream=bf16, out_rows=None):
        """(ops.gemm keywords, gemm_check.resid keywords, the (view, buffer) the launch writes in place or None)"""
        from opendwm_amd import ops
        M, N = self.M, self.N
        R = M if out_rows is None else out_rows
        groups = (M + rpg - 1) // rpg
        base, inplace = form.replace("_inplace", ""), form.endswith("_inplace")
        fill = "sentinel" if inplace else G.NAN
        kw, rk, target = dict(epilogue=ops.EPI_RESID), {}, None
        if base == "gate_res":
            gate, _ = self.operand("gate", (groups, N), 4)
            res, rbuf = self.operand("res", (R, N), 5, stream, fill)
            kw.update(gate=gate, rows_per_gate=rpg, res=res)
            rk.update(gate=gate, rows_per_gate=rpg, res=res.clone())
            target = (res, rbuf)
        elif base == "res_blend":
            res, _ = self.operand("res", (R, N), 5, stream)
            blend, bbuf = self.operand("blend", (R, N), 6, stream, fill)
            alpha, _ = G.fenced_vec(groups, f32, self.dev)
            G.put(alpha, self.data("alpha", (groups,), 7))
            kw.update(res=res, blend=blend, alpha=alpha, rows_per_alpha=rpg)
            rk.update(res=res, blend=blend.clone(), alpha=alpha, rows_per_alpha=rpg)
            target = (blend, bbuf)
        elif base == "res":
            res, rbuf = self.operand("res", (R, N), 5, stream, fill)
            kw.update(res=res)
            rk.update(res=res.clone())
            target = (res, rbuf)
        elif base == "mod_pos":
            pos, _ = self.operand("pos", (rpg, N), 8)
            kw.update(res=pos, res_mod=rpg)
            rk.update(res=pos, res_mod=rpg)
        elif base in ("mod_neg", "mod_neg_relu"):
            per, _ = self.operand("per", (groups, N), 9)
            kw.update(res=per, res_mod=-rpg)
            rk.update(res=per, res_mod=-rpg)
        else:
            raise ValueError(form)
        return kw, rk, (target if inplace else None)

    def run(self, form, *, act="none", rpg=100, tile=0, split_k=1, c32=None, tag=None):
        """c32: None, "mirror", "nomirror" (RESID forms on the fp32 stream).  Returns (ratio, result tensor)."""
        from opendwm_amd import ops
        M, N, K = self.M, self.N, self.K
        tag = tag or dict(form=form, act=act, M=M, N=N, K=K, rpg=rpg, tile=tile, split_k=split_k, c32=c32, rows=bool(self.spare))
        common = dict(tile=tile, split_k=split_k, **self.rows_kw, **self.gemm_kw)
        if form == "plain":
            out, obuf = G.fenced((M, N), bf16, self.dev, col_off=8, pad_cols=8, fill="sentinel")
            ops.gemm(self.a, self.w, self.b, act=_act_code(act), out=out, **common)
            return _verify(out, obuf, G.plain(self.prod, self.b, act), K, tag), out
        if act == "none" and form == "mod_neg_relu":
            act = "relu"
        kw, rk, target = self.resid_operands(form, rpg, f32 if c32 else bf16)
        ref = G.resid(self.prod, self.b, act, **rk)
        if c32 is None:
            out, obuf = target if target else G.fenced((M, N), bf16, self.dev, col_off=8, pad_cols=8, fill="sentinel")
            ops.gemm(self.a, self.w, self.b, act=_act_code(act), out=out, **kw, **common)
            return _verify(out, obuf, ref, K, tag), out
        out32, obuf32 = target if target else G.fenced((M, N), f32, self.dev, col_off=4, pad_cols=4, fill="sentinel")
        assert out32.stride(0) == N + 8
        if c32 == "mirror":
            out, obuf = G.fenced((M, N), bf16, self.dev, col_off=8, pad_cols=8, fill="sentinel")
            ops.gemm(self.a, self.w, self.b, out=out, out32=out32, **kw, **common)
            assert G.untouched(obuf, out), ("mirror fence touched", tag)
            assert torch.equal(out, out32.to(bf16)), ("the bf16 mirror is not the rounded fp32 result", tag)
        else:
            ops.gemm(self.a, self.w, self.b, out32=out32, mirror=False, **kw, **common)
        return _verify(out32, obuf32, ref, K, tag), out32

    def run_geglu(self, tile=0):
        from opendwm_amd import ops
        from opendwm_amd.blocks import geglu_pack
        M, N, K = self.M, self.N, self.K
        wp, _ = G.fenced((N, K), bf16, self.dev, col_off=0, pad_cols=0)
        G.put(wp, geglu_pack(self.w_plain))
        bp, _ = G.fenced_vec(N, bf16, self.dev)
        G.put(bp, geglu_pack(self.b_plain))
        out, obuf = G.fenced((M, N // 2), bf16, self.dev, col_off=8, pad_cols=8, fill="sentinel")
        ops.gemm(self.a, wp, bp, epilogue=ops.EPI_GEGLU, out=out, tile=tile, split_k=1, **self.rows_kw)
        return _verify(out, obuf, G.geglu(self.prod, self.b), K, dict(form="geglu", M=M, N=N, K=K, tile=tile))

    def run_rmshead(self, ncols, tile=0):
        """(worst (row, head) block, element ratio of the columns that are not normalised)"""
        from opendwm_amd import ops
        M, N, K = self.M, self.N, self.K
        rms, _ = G.fenced_vec(ncols, bf16, self.dev)
        G.put(rms, (self.data("rms", (ncols,), 10) * 0.2 + 1).to(bf16))
        out, obuf = G.fenced((M, N), bf16, self.dev, col_off=8, pad_cols=8, fill="sentinel")
        ops.gemm(self.a, self.w, self.b, epilogue=ops.EPI_RMSHEAD, rms_w=rms, rms_ncols=ncols, rms_eps=1e-6, out=out, tile=tile,
                 split_k=1, **self.rows_kw)
        tag = dict(form="rmshead", M=M, N=N, K=K, ncols=ncols, tile=tile)
        assert G.untouched(obuf, out), ("output fence touched", tag)
        assert bool(torch.isfinite(out).all()), ("NaN / Inf in the result", tag)
        block, ratio = G.rmshead_check(out, G.rmshead(self.prod, self.b, rms, ncols, 1e-6), K, ncols)
        assert block < TOL_KERNEL and ratio <= 1, (block, ratio, tag)
        return block, ratio


def _spare(M, N):
    """`rows=` smaller than a.shape[0] on every other shape"""
    return 5 if (M + N // 8) % 2 else 0


# ------------------------------------------------------------------------------------------ W8_256 / W8_128, single pass
@pytest.mark.parametrize("tile", [1, 2])
@pytest.mark.parametrize("M,N,K", PAIRWISE)
def test_plain_and_resid_behind_fences(dev, worst, M, N, K, tile):
    """PLAIN with bias x {none, gelu_tanh, silu, relu} and RESID in the six operand sets of test_gemm_resid + the two in-place
    forms, group sizes 7 (a 16-row MFMA block straddles group seams) and 100, on the 256 x 256 and the 256 x 128 tile"""
    p = Problem(dev, M, N, K, spare=_spare(M, N))
    fam = "W8_256" if tile == 1 else "W8_128"
    for act in ACTS:
        r, _ = p.run("plain", act=act, tile=tile)
        _note(worst, fam, r, form="plain", act=act, M=M, N=N, K=K)
    for rpg in (7, 100):
        for form in RESID_FORMS:
            r, _ = p.run(form, rpg=rpg, tile=tile)
            _note(worst, fam, r, form=form, rpg=rpg, M=M, N=N, K=K)


@pytest.mark.parametrize("tile", [1, 2])
@pytest.mark.parametrize("M,N,K", [(M, N, KS[(i + j) % 3]) for i, M in enumerate(MS) for j, N in enumerate((128, 320))])
def test_geglu_behind_fences(dev, worst, M, N, K, tile):
    r = Problem(dev, M, N, K, spare=_spare(M, N)).run_geglu(tile)
    _note(worst, ("W8_256" if tile == 1 else "W8_128") + "_geglu", r, M=M, N=N, K=K)


@pytest.mark.parametrize("tile", [1, 2])
@pytest.mark.parametrize("M,heads,K", [(M, h, KS[(i + j) % 3]) for i, M in enumerate(MS) for j, h in enumerate((1, 2))])
def test_rmshead_behind_fences(dev, worst, M, heads, K, tile):
    N = 3 * 64 * heads
    block, r = Problem(dev, M, N, K, spare=_spare(M, N)).run_rmshead(2 * 64 * heads, tile)
    _note(worst, ("W8_256" if tile == 1 else "W8_128") + "_rmshead_v", r, M=M, N=N, K=K, worst_head_block=block)


# --------------------------------------------------------------------------------------------------------- automatic tile
@pytest.mark.parametrize("M", [1, 257])
def test_automatic_tile_on_both_sides_of_the_k_flip(dev, worst, M):
    """tile = 0, N = 320: 256 x 128 tiles up to K = 640 (they pad 384 instead of 512 columns), 256 x 256 beyond.  The tiles accumulate
    in the same order, so the explicit configuration the rule predicts must agree bit for bit."""
    for K, predicted in ((640, 2), (704, 1)):
        p = Problem(dev, M, 320, K, spare=5)
        for form in ("plain", "gate_res"):
            r, auto = p.run(form, tile=0)
            _note(worst, "automatic_tile", r, form=form, M=M, N=320, K=K)
            _, explicit = p.run(form, tile=predicted)
            assert torch.equal(auto, explicit), (K, form)


# ---------------------------------------------------------------------------------------------------------------- split-K
@pytest.mark.parametrize("M,N", [(1, 8), (1, 264), (257, 8), (257, 264)])
def test_split_k_behind_fences(dev, worst, M, N):
    """K = 1024 in 2 ranges (8 + 8 steps), K = 1088 in 2 ranges (17 steps: 8 + 9, the uneven cut no other test has), and
    K = 1088 with the automatic rule: at most 4 tiles -> 256 / tiles >= 64 ranges, clamped to 17 / 8 = 2 - the same 2 ranges, so it
    must be bit-equal to the explicit split.  Twice, bit-equal (fixed reduction order)."""
    for K, split in ((1024, 2), (1088, 2), (1088, 0)):
        p = Problem(dev, M, N, K, spare=_spare(M, N))
        for form in ("plain", "gate_res_inplace", "mod_neg"):
            r, first = p.run(form, split_k=split)
            first = first.clone()
            _note(worst, "W8_SPLITK", r, form=form, M=M, N=N, K=K, split_k=split)
            _, again = p.run(form, split_k=split)
            assert torch.equal(first, again), (K, split, form)
            if split == 0:
                _, explicit = p.run(form, split_k=2)
                assert torch.equal(first, explicit), ("the automatic rule did not take 2 ranges", form)


# ------------------------------------------------------------------------------------------------------ fp32 residual stream
@pytest.mark.parametrize("M,N,K,rpg", [(257, 264, 128, 100), (1, 8, 64, 7), (256, 128, 192, 7), (255, 136, 64, 100)])
def test_fp32_stream_behind_fences(dev, worst, M, N, K, rpg):
    """W8_C32: fp32 res / blend / out32 fenced (ldc32 = N + 8), with and without the bf16 mirror, out of place and in place over
    res and over blend; out32 against the fp32 bound, the mirror equal to out32 rounded"""
    p = Problem(dev, M, N, K, spare=5 if M == 257 else 0)
    for c32 in ("mirror", "nomirror"):
        for form in ("gate_res", "res_blend", "res", "gate_res_inplace", "res_blend_inplace", "res_inplace"):
            r, _ = p.run(form, rpg=rpg, c32=c32)
            _note(worst, "W8_C32", r, form=form, c32=c32, M=M, N=N, K=K, rpg=rpg)


# ------------------------------------------------------------------------------------------------------------------ 4-wave
def _counters():
    from opendwm_amd import _lib
    lib = _lib.load()
    return int(lib.dwm_gemm4w_launches()), int(lib.dwm_gemm4w_launches_general())


def _up(n, q):
    return (n + q - 1) // q * q


@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (512, 256, 192), (257, 264, 128), (255, 136, 192), (1, 8, 128)])
def test_four_wave_behind_fences(dev, worst, M, N, K):
    """inside ops.gemm_4wave_scope (per thread: no subprocess needed): the fast form at M % 256 == N % 256 == 0, the general form
    at ragged sizes - asserted through the deltas of the two launch counters.  GEGLU and the q / k heads need N % 64 == 0: at the
    ragged shapes they run at N rounded up to 64 (still ragged against the 256-column tile)."""
    from opendwm_amd import ops
    fast = M % 256 == 0 and N % 256 == 0
    fam = "W4_FAST" if fast else "W4_GENERAL"
    p = Problem(dev, M, N, K, spare=5)
    n64 = _up(N, 64)
    p64 = p if n64 == N else Problem(dev, M, n64, K, spare=5)
    ncols = max(64, (n64 // 64) * 2 // 3 * 64)
    with ops.gemm_4wave_scope(True):
        n0 = _counters()
        for act in ACTS:
            r, _ = p.run("plain", act=act)
            _note(worst, fam, r, form="plain", act=act, M=M, N=N, K=K)
        r = p64.run_geglu()
        _note(worst, fam, r, form="geglu", M=M, N=n64, K=K)
        block, r = p64.run_rmshead(ncols)
        _note(worst, fam, r, form="rmshead_v", M=M, N=n64, K=K, worst_head_block=block)
        for form in ("res", "gate_res", "res_blend", "gate_res_inplace", "res_blend_inplace"):      # RS 2, 3, 6
            r, _ = p.run(form, rpg=7)
            _note(worst, fam, r, form=form, M=M, N=N, K=K)
        for form in ("res", "gate_res", "res_blend", "res_inplace"):                                  # fp32 stream, no mirror
            r, _ = p.run(form, rpg=100, c32="nomirror")
            _note(worst, fam, r, form=form, c32="nomirror", M=M, N=N, K=K)
        n1 = _counters()
        assert (n1[0] - n0[0], n1[1] - n0[1]) == (15, 0 if fast else 15), (n0, n1)
        r, _ = p.run("mod_neg", rpg=7)                     # RS 18: the per-image residual row exists in the general form only
        _note(worst, "W4_GENERAL", r, form="mod_neg", M=M, N=N, K=K)
        n2 = _counters()
        assert (n2[0] - n1[0], n2[1] - n1[1]) == (1, 1), (n1, n2)


@pytest.mark.parametrize("M,N", [(257, 264), (256, 256)])
def test_four_wave_uncovered_neighbours_stay_eight_wave(dev, worst, M, N):
    """one K step, res_mod > 0, RESID with an activation, out32 with the bf16 mirror: both counters stay, and the 8-wave kernels
    that answer inside the scope pass the same fences and bounds"""
    from opendwm_amd import ops
    with ops.gemm_4wave_scope(True):
        n0 = _counters()
        p = Problem(dev, M, N, 64, spare=5)
        for form, kw in (("plain", dict(act="silu")), ("gate_res", {}), ("res", dict(c32="nomirror"))):
            r, _ = p.run(form, **kw)
            _note(worst, "W4_declined", r, form=form, M=M, N=N, K=64, **kw)
        p = Problem(dev, M, N, 128, spare=5)
        for form, kw in (("mod_pos", {}), ("res", dict(act="silu")), ("gate_res", dict(act="gelu_tanh")), ("gate_res", dict(c32="mirror")),
                         ("res_blend_inplace", dict(c32="mirror"))):
            r, _ = p.run(form, rpg=7, **kw)
            _note(worst, "W4_declined", r, form=form, M=M, N=N, K=128, **kw)
        assert _counters() == n0


# ------------------------------------------------------------------------------------- implicit 3x3 convolution with c_grid
@pytest.mark.parametrize("C,N,tile,split_k", [(64, 72, 1, 1), (64, 192, 1, 1), (64, 72, 2, 1), (64, 192, 2, 1),
                                              (128, 72, 0, 2), (128, 192, 0, 2),          # K = 1152: 18 steps, 9 + 9
                                              (192, 72, 0, 3), (192, 192, 0, 3),          # K = 1728: 27 steps, 9 + 9 + 9
                                              (192, 72, 0, 2), (192, 192, 0, 2)])         # ... 13 + 14: the uneven cut, across a tap
def test_implicit_conv_padded_output_behind_fences(dev, worst, C, N, tile, split_k):
    """3x3 convolution as implicit GEMM from a padded token grid (NaN-fenced rows before and after it) into a padded output grid
    whose border rows and fence hold the sentinel: both must stay untouched bit for bit (a zero border that stays zero says
    nothing about a store of zeros).  PLAIN + silu, and RESID in place over the padded residual."""
    from opendwm_amd import ops
    I, h, w = 2, 4, 6
    grid = ops.PaddedGrid(I, h, w)
    idx = grid.interior_index().to(dev)
    M, K = grid.pixels, 9 * C
    xp, _ = G.fenced((grid.rows, C), bf16, dev, col_off=16, pad_cols=48)
    xp.zero_()
    xp[idx] = _rand((M, C), dev, 1)
    shifts = torch.tensor(grid.tap_shifts(), device=dev)
    a_full = xp[idx[:, None] + shifts[None, :]].reshape(M, K)          # the im2col matrix the kernel never builds
    p = Problem(dev, M, N, K, a=a_full)
    border = torch.ones(grid.rows, dtype=torch.bool, device=dev)
    border[idx] = False
    fam = "conv3x3_c_grid" + ("_splitk" if split_k > 1 else "")
    conv = dict(a_grid=grid, conv3x3=True, c_grid=grid, tile=tile, split_k=split_k)
    tag = dict(C=C, N=N, tile=tile, split_k=split_k)

    def verify(out, obuf, ref, form):
        assert G.untouched(obuf, out), ("output fence touched", form, tag)
        assert G.holds_fill(out[border]), ("border rows of the padded output written", form, tag)
        inner = out[idx]
        assert bool(torch.isfinite(inner).all()), ("NaN / Inf in the result", form, tag)
        ratio = G.check(inner, ref, K)
        if not ratio <= 1:
            for line in G.worst(inner, ref, K):
                print("   ", line)
        assert ratio <= 1, (ratio, form, tag)
        _note(worst, fam, ratio, form=form, **tag)

    out, obuf = G.fenced((grid.rows, N), bf16, dev, col_off=8, pad_cols=8, fill="sentinel")
    ops.gemm(xp, p.w, p.b, act=ops.ACT_SILU, out=out, **conv)
    verify(out, obuf, G.plain(p.prod, p.b, "silu"), "plain_silu")
    res, rbuf = G.fenced((grid.rows, N), bf16, dev, col_off=8, pad_cols=8, fill="sentinel")
    r0 = _rand((M, N), dev, 5)
    res[idx] = r0
    ops.gemm(xp, p.w, p.b, epilogue=ops.EPI_RESID, res=res, out=res, **conv)
    verify(res, rbuf, G.resid(p.prod, p.b, res=r0), "res_inplace")


# ------------------------------------------------------------------------------------------------------------ dwm_gemm_tn
TN_M, TN_N, TN_C, TN_SPLIT = (64, 128, 192), (8, 72, 136), (8, 72, 264), (1, 2, 0)
# two orthogonal Latin squares over the 9 (M, N) pairs: every pair of values of any two of the four factors occurs
TN_CASES = [(M, N, TN_C[(i + j) % 3], TN_SPLIT[(i + 2 * j) % 3]) for i, M in enumerate(TN_M) for j, N in enumerate(TN_N)]
# dwm_gemm_tn wants >= 8 K steps of 64 rows per range: the shapes above take one range only (split_k = 2 is refused, see below);
# these two really split - 16 steps in 8 + 8 and 17 steps in 8 + 9
TN_CASES += [(1024, 72, 72, 2), (1088, 136, 264, 2), (1088, 8, 8, 0)]


@pytest.mark.parametrize("taps", [None, (-1, 0, 1)], ids=["no_taps", "three_taps"])
@pytest.mark.parametrize("M,N,C,split_k", TN_CASES)
def test_gemm_tn_behind_fences(dev, worst, M, N, C, split_k, taps):
    """out[n, t*C + c] = sum_m dy[m, n] x[clamp(m + shift_t, 0, rows - 1), c] against fp64 on the same clamp; with taps x has as
    many rows as dy, so the clamp acts at both ends.  dy and x fenced views, out fenced with ldo = cols + 16; the bound with
    K -> M.  A range count the contraction is too short for (fewer than 8 steps of 64 rows per range) is refused and nothing is
    written."""
    from opendwm_amd import train_ops as T
    dy, _ = G.fenced((M, N), bf16, dev, col_off=8, pad_cols=8)
    x, _ = G.fenced((M, C), bf16, dev, col_off=8, pad_cols=8)
    G.put(dy, _rand((M, N), dev, 1, M ** -0.5))
    G.put(x, _rand((M, C), dev, 2))
    nt = len(taps) if taps else 1
    out, obuf = G.fenced((N, nt * C), bf16, dev, col_off=8, pad_cols=8, fill="sentinel")
    assert out.stride(0) == nt * C + 16
    kw = dict(tap_shifts=list(taps)) if taps else {}
    if split_k > max(1, (M // 64) // 8):
        with pytest.raises(RuntimeError):
            T.gemm_tn(dy, x, split_k=split_k, out=out, **kw)
        torch.cuda.synchronize()
        assert G.holds_fill(obuf)
        return
    T.gemm_tn(dy, x, split_k=split_k, out=out, **kw)
    rows = torch.arange(M, device=dev)
    refs, mags = [], []
    for sh in (taps or (0,)):
        xs = x.double()[(rows + sh).clamp(0, M - 1)]
        refs.append(dy.double().T @ xs)
        mags.append(dy.double().abs().T @ xs.abs())
    ref = G.Ref(torch.cat(refs, 1), torch.cat(mags, 1))
    r = _verify(out, obuf, ref, M, dict(form="gemm_tn", M=M, N=N, C=C, split_k=split_k, taps=taps))
    _note(worst, "gemm_tn", r, M=M, N=N, C=C, split_k=split_k, taps=bool(taps))
    again, abuf = G.fenced((N, nt * C), bf16, dev, col_off=8, pad_cols=8, fill="sentinel")
    T.gemm_tn(dy, x, split_k=split_k, out=again, **kw)
    assert torch.equal(out, again) and G.untouched(abuf, again)
