"""GPU leg of the adapter kernels (csrc/lora.hip): dwm_lora_merge_multi and dwm_lora_project_multi element by element inside the fp64
bounds of tests/lora_ref.py (tests/test_lora_cpu.py shows that a correct fp32 evaluation stays inside them and a wrong one does
not), and the consequences of the normative arithmetic bit for bit: B == 0 is the cast, the bf16 rounding of the fold is the merge,
two launches agree, a list agrees with its entries launched alone.

Every source sits between NaN fences and every output between sentinel fences (tests/gemm_check.py), so a read or a store one
element outside a tensor shows."""
import pytest
import torch

from tests import gemm_check as G
from tests import lora_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.quick]
bf16, f32 = torch.bfloat16, torch.float32
_INT = {bf16: torch.int16, f32: torch.int32}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def src(t, dev):
    """a contiguous copy of the CPU tensor `t` on the device with NaN on both sides"""
    view, _ = G.fenced_vec(t.numel(), t.dtype, dev, off=16)
    view.copy_(t.reshape(-1))
    return view.view(t.shape)


def dst(shape, dtype, dev):
    """(contiguous output view, its buffer): the sentinel pattern everywhere"""
    n = 1
    for s in shape:
        n *= s
    view, buf = G.fenced_vec(n, dtype, dev, off=16, fill="sentinel")
    return view.view(shape), buf


def bits(t):
    return t.contiguous().view(_INT[t.dtype]).cpu()


@pytest.fixture(scope="module")
def cases(dev):
    """(N, K, r, w dtype) -> the CPU operands and their fenced device copies, made once"""
    out = {}
    for N in R.NS:
        for K in R.KS:
            for r in R.RS:
                for wd in (f32, bf16):
                    W, A, B, Gr = R.operands(N, K, r, 1000 + N + 7 * K + 13 * r, wd)
                    out[(N, K, r, wd)] = dict(cpu=(W, A, B, Gr), W=src(W, dev), A=src(A, dev), B=src(B, dev), G=src(Gr, dev))
    return out


S = 0.75            # the scale of most cases (alpha / rank is a power of two in the defaults; this one is not)


@pytest.mark.parametrize("wd", [f32, bf16], ids=["w32", "wbf16"])
@pytest.mark.parametrize("N", R.NS)
def test_merge_and_fold_inside_the_bound_and_consistent(dev, cases, N, wd):
    from opendwm_amd import ops, train_ops as T
    worst = (0.0, None)
    for K in R.KS:
        for r in R.RS:
            c = cases[(N, K, r, wd)]
            W, A, B, _ = c["cpu"]
            exact, mag = R.merge_exact(W, A, B, S)
            merged, mbuf = dst((N, K), bf16, dev)
            T.lora_merge_multi([c["W"]], [c["A"]], [c["B"]], [merged], [S])
            folded, fbuf = dst((N, K), wd, dev)
            T.lora_merge_multi([c["W"]], [c["A"]], [c["B"]], [folded], [S])
            assert G.untouched(mbuf, merged) and G.untouched(fbuf, folded), ("output fence touched", N, K, r)
            for got, name in ((merged, "merge"), (folded, "fold")):
                q = R.ratio(got, exact, R.merge_bound(exact, mag, r, got.dtype))
                assert q <= 1, (name, q, N, K, r, wd)
                if q > worst[0]:
                    worst = (q, (name, N, K, r))
            # the bf16 rounding of the fp32 fold is the merge
            fold32, _ = dst((N, K), f32, dev)
            T.lora_merge_multi([c["W"]], [c["A"]], [c["B"]], [fold32], [S])
            assert torch.equal(bits(ops.cast_bf16(fold32)), bits(merged)), (N, K, r)
            # two launches agree
            again, _ = dst((N, K), bf16, dev)
            T.lora_merge_multi([c["W"]], [c["A"]], [c["B"]], [again], [S])
            assert torch.equal(bits(again), bits(merged))
            # B == 0: the cast
            zero = src(torch.zeros(N, r), dev)
            plain, pbuf = dst((N, K), bf16, dev)
            T.lora_merge_multi([c["W"]], [c["A"]], [zero], [plain], [S])
            want = ops.cast_bf16(c["W"].contiguous()) if wd == f32 else c["W"]
            assert G.untouched(pbuf, plain) and torch.equal(bits(plain), bits(want)), (N, K, r)
    print(f"lora merge N = {N} {wd}: worst element ratio {worst[0]:.3f} at {worst[1]}")


def test_fold_in_place_and_back(dev, cases):
    """out == w (what fold_into_ launches), then the negative scale: back to within one rounding of the element's size"""
    from opendwm_amd import train_ops as T
    for key in ((200, 1536, 16, f32), (7, 60, 4, f32), (64, 192, 64, bf16)):
        c = cases[key]
        W, A, B, _ = c["cpu"]
        N, K, r, wd = key
        w, buf = dst((N, K), wd, dev)
        w.copy_(c["W"])
        T.lora_merge_multi([w], [c["A"]], [c["B"]], [w], [S])
        exact, mag = R.merge_exact(W, A, B, S)
        assert G.untouched(buf, w) and R.ratio(w, exact, R.merge_bound(exact, mag, r, wd)) <= 1
        folded = w.clone()
        T.lora_merge_multi([w], [c["A"]], [c["B"]], [w], [-S])
        assert G.untouched(buf, w)
        # both launches form the same s B A; what is left are their two roundings, half an ulp of the folded and of the restored value
        eps = 2.0 ** -23 if wd == f32 else 2.0 ** -7
        size = torch.maximum(folded.double().abs(), c["W"].double().abs()).cpu()
        assert bool(((w.double().cpu() - W.double()).abs() <= eps * size * (1 + 2.0 ** -6)).all()), key


@pytest.mark.parametrize("accumulate", [False, True], ids=["assign", "accumulate"])
@pytest.mark.parametrize("gd", [f32, bf16], ids=["g32", "gbf16"])
@pytest.mark.parametrize("N", R.NS)
def test_project_inside_the_bound_and_repeatable(dev, cases, N, gd, accumulate):
    from opendwm_amd import train_ops as T
    worst = (0.0, None)
    for K in R.KS:
        for r in R.RS:
            c = cases[(N, K, r, gd)]
            _, A, B, Gr = c["cpu"]
            g = torch.Generator().manual_seed(N + K + r)
            old_a = torch.randn(r, K, generator=g) * 0.01 if accumulate else None
            old_b = torch.randn(N, r, generator=g) * 0.01 if accumulate else None
            (ea, ma), (eb, mb) = R.project_exact(Gr, A, B, S, old_a, old_b)
            outs = []
            for _ in range(2):
                dA, abuf = dst((r, K), f32, dev)
                dB, bbuf = dst((N, r), f32, dev)
                if accumulate:
                    dA.copy_(old_a)
                    dB.copy_(old_b)
                T.lora_project_multi([c["G"]], [c["A"]], [c["B"]], [dA], [dB], [S], accumulate=accumulate)
                assert G.untouched(abuf, dA) and G.untouched(bbuf, dB), ("output fence touched", N, K, r)
                outs.append((dA, dB))
            assert torch.equal(bits(outs[0][0]), bits(outs[1][0])) and torch.equal(bits(outs[0][1]), bits(outs[1][1])), (N, K, r)
            qa = R.ratio(outs[0][0], ea, R.project_bound(ma, N))
            qb = R.ratio(outs[0][1], eb, R.project_bound(mb, K))
            assert qa <= 1 and qb <= 1, (qa, qb, N, K, r, gd, accumulate)
            if max(qa, qb) > worst[0]:
                worst = (max(qa, qb), (N, K, r))
    print(f"lora project N = {N} {gd} accumulate = {accumulate}: worst element ratio {worst[0]:.3f} at {worst[1]}")


def test_project_sums_more_than_one_row_chunk_in_order(dev):
    """N = 1100 is three partials of at most 512 rows: the finishing launch adds them in ascending order (checked on the
    partials themselves), inside the bound, twice the same"""
    from opendwm_amd import train_ops as T
    N, K, r = 1100, 132, 5
    _, A, B, Gr = R.operands(N, K, r, 77)
    d = dict(A=src(A, dev), B=src(B, dev), G=src(Gr, dev))
    dA, abuf = dst((r, K), f32, dev)
    dB, bbuf = dst((N, r), f32, dev)
    parts = T.lora_project_multi([d["G"]], [d["A"]], [d["B"]], [dA], [dB], [S], return_partials=True)[0]
    assert tuple(parts.shape) == (3, r, K) and G.untouched(abuf, dA) and G.untouched(bbuf, dB)
    assert torch.equal(bits(dA), bits(((parts[0] + parts[1]) + parts[2]) * S))
    (ea, ma), (eb, mb) = R.project_exact(Gr, A, B, S)
    assert R.ratio(dA, ea, R.project_bound(ma, N)) <= 1 and R.ratio(dB, eb, R.project_bound(mb, K)) <= 1
    # every partial is its own chunk's sum
    for ci in range(3):
        rows = slice(512 * ci, min(512 * (ci + 1), N))
        (pe, pm), _ = R.project_exact(Gr[rows], A, B[rows], 1.0)
        assert R.ratio(parts[ci], pe, R.project_bound(pm, 512)) <= 1, ci


def test_lists_of_mixed_shapes_equal_their_entries(dev, cases):
    from opendwm_amd import train_ops as T
    keys = [(200, 1536, 16, f32), (1, 4, 1, f32), (7, 60, 64, bf16), (64, 192, 4, f32), (200, 64, 16, bf16), (64, 1536, 64, f32)]
    cs = [cases[k] for k in keys]
    scales = [0.5 + 0.25 * i for i in range(len(keys))]
    Ws, As, Bs, Gs = ([c[n] for c in cs] for n in "WABG")
    # merge: fp32 weights to bf16 (the merge), bf16 weights to bf16
    outs = [dst((k[0], k[1]), bf16, dev) for k in keys]
    T.lora_merge_multi(Ws, As, Bs, [o for o, _ in outs], scales)
    for k, c, s, (o, buf) in zip(keys, cs, scales, outs):
        alone, _ = dst((k[0], k[1]), bf16, dev)
        T.lora_merge_multi([c["W"]], [c["A"]], [c["B"]], [alone], [s])
        assert G.untouched(buf, o) and torch.equal(bits(o), bits(alone)), k
    dAs = [dst((k[2], k[1]), f32, dev) for k in keys]
    dBs = [dst((k[0], k[2]), f32, dev) for k in keys]
    T.lora_project_multi(Gs, As, Bs, [o for o, _ in dAs], [o for o, _ in dBs], scales)
    for k, c, s, (da, abuf), (db, bbuf) in zip(keys, cs, scales, dAs, dBs):
        a1, _ = dst((k[2], k[1]), f32, dev)
        b1, _ = dst((k[0], k[2]), f32, dev)
        T.lora_project_multi([c["G"]], [c["A"]], [c["B"]], [a1], [b1], [s])
        assert G.untouched(abuf, da) and G.untouched(bbuf, db), k
        assert torch.equal(bits(da), bits(a1)) and torch.equal(bits(db), bits(b1)), k


def test_unsupported_shapes_are_refused(dev):
    from opendwm_amd import train_ops as T
    z = lambda *s: torch.zeros(*s, device=dev)
    for N, K, r in ((8, 64, 65), (8, 6, 2)):
        with pytest.raises(RuntimeError, match="DWM_EUNSUPPORTED"):
            T.lora_merge_multi([z(N, K)], [z(r, K)], [z(N, r)], [torch.empty(N, K, dtype=bf16, device=dev)], [1.0])
        with pytest.raises(RuntimeError, match="DWM_EUNSUPPORTED"):
            T.lora_project_multi([z(N, K)], [z(r, K)], [z(N, r)], [z(r, K)], [z(N, r)], [1.0])
