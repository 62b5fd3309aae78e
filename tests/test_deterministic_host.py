"""Deterministic mode, the part that needs no GPU: the public surface, the context manager's state handling and the plan query of
the deterministic weight gradient (tv_wgrad_tn_plan: host arithmetic, documented layout in include/transvae_hip.h)."""
import ctypes as C
import inspect

import pytest


def test_exports_and_signatures():
    import transvae
    from transvae.hip import ops
    assert "deterministic" in transvae.__all__ and transvae.deterministic is ops.deterministic
    assert list(inspect.signature(ops.set_deterministic).parameters) == ["on"]
    assert list(inspect.signature(ops.is_deterministic).parameters) == []
    p = inspect.signature(ops.deterministic).parameters
    assert list(p) == ["on"] and p["on"].default is True
    assert callable(ops.det_workspace)
    assert ops.is_deterministic() is False          # off unless asked for


def test_context_manager_restores_state():
    from transvae.hip import ops
    assert not ops.is_deterministic()
    with ops.deterministic():
        assert ops.is_deterministic()
        with ops.deterministic(False):
            assert not ops.is_deterministic()
        assert ops.is_deterministic()
    assert not ops.is_deterministic()
    with pytest.raises(KeyError):
        with ops.deterministic():
            raise KeyError("boom")
    assert not ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        with pytest.raises(KeyError):
            with ops.deterministic(False):
                assert not ops.is_deterministic()
                raise KeyError("boom")
        assert ops.is_deterministic()               # the PREVIOUS state, not "off"
    finally:
        ops.set_deterministic(False)
    assert not ops.is_deterministic()


def _linear(T, c_in, c_out):
    from transvae.hip import ops
    return ops._rows_desc(T, c_in, c_out)


def _c3s1(B, H, W, c_in, c_out):
    from transvae.hip import ops
    return ops._desc(batch=B, h_in=H, w_in=W, c_in=c_in, ldx=c_in, h_out=H, w_out=W, c_out=c_out, ldo=c_out, kh=3, kw=3, pad=1)


def _plan(desc, accum=0):
    from transvae.hip import _lib as L
    ny, nbytes = C.c_int(-1), C.c_longlong(-1)
    assert L.load().tv_wgrad_tn_plan(C.byref(desc), accum, C.byref(ny), C.byref(nbytes)) == 0
    return ny.value, nbytes.value


def test_plan_single_chunk_needs_no_workspace():
    assert _plan(_linear(512, 64, 64)) == (1, 0)
    assert _plan(_linear(512, 64, 64), 1) == (1, 0)


@pytest.mark.parametrize("desc", [_linear(4096, 384, 192), _c3s1(4, 64, 64, 192, 384)], ids=["linear-4096x384-192", "c3s1-4x64x64x192-384"])
def test_plan_workspace_follows_the_documented_layout(desc):
    """ny weight slices of c_out * taps * c_in floats, then ny bias slices of c_out floats"""
    answers = [_plan(desc, a) for a in (0, 1, 0, 1, 0)]
    assert len(set(answers)) == 1, answers          # the same answer on every call, whatever `accum`
    ny, nbytes = answers[0]
    assert ny > 1
    assert nbytes == ny * (desc.c_out * desc.kh * desc.kw * desc.c_in + desc.c_out) * 4


def test_plan_rejects_bad_arguments():
    from transvae.hip import _lib as L
    lib = L.load()
    d = _linear(512, 60, 64)                        # c_in must be a multiple of 8
    ny, nbytes = C.c_int(0), C.c_longlong(0)
    assert lib.tv_wgrad_tn_plan(C.byref(d), 0, C.byref(ny), C.byref(nbytes)) != 0
    assert lib.tv_wgrad_tn_plan(C.byref(_linear(512, 64, 64)), 0, None, C.byref(nbytes)) != 0


def test_scratch_query_of_the_rownorm_backward():
    from transvae.hip import _lib as L
    lib = L.load()
    assert lib.tv_rownorm_bwd_det_scratch_bytes(65, 72) == 17 * 72 * 4            # one workgroup per four rows ...
    assert lib.tv_rownorm_bwd_det_scratch_bytes(1 << 20, 384) == 1024 * 384 * 4   # ... 1024 at the most
    assert lib.tv_rownorm_bwd_det_scratch_bytes(0, 384) < 0
