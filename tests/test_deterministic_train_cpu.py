"""CPU leg of the order-deterministic training mode: the ordered entry points and their size queries are declared in the
header and bound in _lib.SIGNATURES without an ABI bump, CTSDTrainer takes `deterministic`, and the per-thread scope nests, restores
and travels from a Function's forward to its backward on another thread."""
import inspect
import os
import re
import threading

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ["segsum", "segsum_diff", "layernorm_bwd", "rmsnorm_heads_bwd", "groupnorm_bwd"]


def _header():
    return open(os.path.join(ROOT, "include", "dwm_hip.h")).read()


def test_ordered_symbols_declared_and_bound():
    from opendwm_amd import _lib
    h = _header()
    for op in OPS:
        for sym, ret in ((f"dwm_{op}_ordered", "int"), (f"dwm_{op}_ordered_floats", "int64_t")):
            assert re.search(rf"^{ret} {sym}\(", h, re.M), sym
            assert sym in _lib.SIGNATURES, sym
        res, args = _lib.SIGNATURES[f"dwm_{op}_ordered"]
        res0, args0 = _lib.SIGNATURES[f"dwm_{op}"]
        # the sibling's arguments + (workspace, workspace_floats) in front of the stream
        assert res is res0 and list(args) == list(args0[:-1]) + [_lib._vp, _lib._i64, args0[-1]], op
        assert _lib.SIGNATURES[f"dwm_{op}_ordered_floats"][0] is _lib._i64
    # the header says what the tests re-implement: chunk sizes and the fold order
    assert "plain left fold over ASCENDING chunk index" in h
    for word in ("[groups][cpg][ncols]", "[slots][groups][cpg][D]", "[chunks][ncols]", "[I][chunks][2][C]"):
        assert word in h, word


def test_abi_version_is_still_18():
    from opendwm_amd import _lib
    assert _lib.ABI_VERSION == 18
    assert re.search(r"^#define DWM_ABI_VERSION 18$", _header(), re.M)
    # additions only: the existing struct and signatures are as they were
    assert "float* dgamma; float* dbeta; float* dgamma2; float* dbeta2; int64_t ld_grad; int32_t grad_per_group;\n} dwm_layernorm_bwd_args;" in _header()
    assert len(_lib.SIGNATURES["dwm_segsum"][1]) == 10 and len(_lib.SIGNATURES["dwm_groupnorm_bwd"][1]) == 18


def test_size_queries_on_the_host():
    """the queries are host arithmetic: callable without a device, and equal to the documented chunking"""
    from opendwm_amd import _lib
    lib = _lib.load()
    assert lib.dwm_segsum_ordered_floats(1001, 1536, 154) == 7 * 2 * 1536
    assert lib.dwm_segsum_diff_ordered_floats(129, 8, 129) == 2 * 8
    assert lib.dwm_segsum_ordered_floats(5, 8, 1000) == 8            # rows_per_group beyond the rows: one group, one chunk
    assert lib.dwm_rmsnorm_heads_bwd_ordered_floats(333, 3072) == 11 * 3072
    a = _lib.LayerNormBwdArgs()
    a.rows, a.D, a.rows_per_mod = 5 * 77, 320, 77
    assert lib.dwm_layernorm_bwd_ordered_floats(a) == 0             # no accumulator, no partials
    a.dgamma, a.dbeta2 = 16, 32                                       # any non-null pointers: two slots
    assert lib.dwm_layernorm_bwd_ordered_floats(a) == 2 * 5 * 2 * 320
    a.rows_per_mod = 0
    assert lib.dwm_layernorm_bwd_ordered_floats(a) == 2 * 7 * 320    # one group of 385 rows: 7 chunks of 64
    n = lib.dwm_groupnorm_bwd_ordered_floats(12, 48, 320)
    assert n == 12 * 1 * 2 * 320                                     # 48 pixels: one statistics chunk per image
    assert lib.dwm_segsum_ordered_floats(0, 8, 1) == 0 and lib.dwm_groupnorm_bwd_ordered_floats(1, 0, 8) == 0


def test_trainer_accepts_deterministic():
    from opendwm_amd.pipeline import CTSDTrainer
    p = inspect.signature(CTSDTrainer.__init__).parameters["deterministic"]
    assert p.default is False
    for name in ("return_partials",):
        from opendwm_amd import train_ops as T
        for fn in (T.segsum, T.segsum_diff, T.layernorm_bwd, T.rmsnorm_heads_bwd_, T.groupnorm_bwd):
            assert inspect.signature(fn).parameters[name].default is False


def test_scope_nests_and_restores():
    from opendwm_amd import train_ops as T
    assert not T.ordered_reductions_enabled()
    with T.ordered_reductions(True):
        assert T.ordered_reductions_enabled()
        with T.ordered_reductions(False):
            assert not T.ordered_reductions_enabled()
            with T.ordered_reductions(True):
                assert T.ordered_reductions_enabled()
            assert not T.ordered_reductions_enabled()
        assert T.ordered_reductions_enabled()
        seen = []
        t = threading.Thread(target=lambda: seen.append(T.ordered_reductions_enabled()))
        t.start(); t.join()
        assert seen == [False]                    # per thread: another thread starts outside the scope
    assert not T.ordered_reductions_enabled()
    try:
        with T.ordered_reductions(True):
            raise KeyError("x")
    except KeyError:
        pass
    assert not T.ordered_reductions_enabled()    # restored on the way out of an exception too


def _fn(decorator):
    from opendwm_amd import train_ops as T
    seen = {}

    @decorator
    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            seen["fwd"] = T.ordered_reductions_enabled()
            return x * 2

        @staticmethod
        def backward(ctx, g):
            seen["bwd"] = (T.ordered_reductions_enabled(), threading.get_ident())
            return g * 2
    return Fn, seen


def test_decorated_function_reopens_the_scope_on_another_thread():
    from opendwm_amd import ops, train_ops as T
    for deco in (ops.carries_ordered_scope, ops.carries_gemm_scope):
        for on in (True, False):
            Fn, seen = _fn(deco)
            x = torch.ones(3, requires_grad=True)
            with T.ordered_reductions(on):
                y = Fn.apply(x).sum()
            assert seen["fwd"] is on
            t = threading.Thread(target=y.backward)          # outside the scope, on a thread that never saw it
            t.start(); t.join()
            assert seen["bwd"] == (on, t.ident) and t.ident != threading.get_ident()
            assert torch.equal(x.grad, torch.full((3,), 2.0))
            assert not T.ordered_reductions_enabled()


def test_gemm_scope_is_still_carried_beside_it():
    from opendwm_amd import ops
    got = {}

    @ops.carries_gemm_scope
    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x + 1

        @staticmethod
        def backward(ctx, g):
            got["g4w"], got["ord"] = ops.gemm_4wave_enabled(), ops.ordered_reductions_enabled()
            return g
    x = torch.ones(2, requires_grad=True)
    with ops.gemm_4wave_scope(True):
        y = Fn.apply(x).sum()
    y.backward()
    assert got == dict(g4w=True, ord=False)


def test_training_forwards_open_the_scope_from_the_model_attribute():
    from opendwm_amd import ops, train, train_unet

    class M:
        pass
    seen = []
    probe = ops.opens_ordered_scope(lambda model, *a: seen.append(ops.ordered_reductions_enabled()))
    m = M()
    probe(m)
    m.ordered_reductions = True
    probe(m)
    m.ordered_reductions = False
    probe(m)
    assert seen == [False, True, False] and not ops.ordered_reductions_enabled()
    for f in (train.forward_train, train_unet.forward_train):
        assert hasattr(f, "__wrapped__") and list(inspect.signature(f).parameters)[:2] == ["model", "sample"]
    for name, cls in vars(train_unet).items():
        if inspect.isclass(cls) and issubclass(cls, torch.autograd.Function) and cls.__module__ == train_unet.__name__:
            assert cls.backward.__qualname__.startswith("carries_ordered_scope"), name
