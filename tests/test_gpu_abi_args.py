"""GPU: the typed pointer arguments of `_lib.SIGNATURES` change nothing about a call -- a tensor
and its integer address give the same bytes -- and what they reject is rejected on the host,
before the library is entered: no call here hands the library a bad address."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _exp10_inputs():
    import torch
    x = torch.linspace(-30., 30., 64, dtype=torch.float64, device="cuda")
    return torch, x


def test_exp10_tensors_and_addresses_give_the_same_bytes():
    from brutus_amd import _lib
    torch, x = _exp10_inputs()
    L = _lib.lib()
    y_t, y_a = torch.full_like(x, -1.), torch.full_like(x, -2.)
    _lib.check(L.brutus_debug_exp10(x, y_t, 64, None))
    _lib.check(L.brutus_debug_exp10(x.data_ptr(), y_a.data_ptr(), 64, None))
    torch.cuda.synchronize()
    got = y_t.cpu().numpy()
    assert got.tobytes() == y_a.cpu().numpy().tobytes()
    assert np.allclose(got, 10. ** x.cpu().numpy(), rtol=1e-13)     # (and the call did run)


def test_los_loglike_through_the_class_and_by_addresses():
    """Optional pointers (None), a typed struct and an untyped workspace in one call: 3 objects
    x 2 draws, 1 cloud, 2 thetas."""
    import torch
    from brutus_amd import _lib, los
    ds = np.array([[6.1, 6.4], [9.3, 9.0], [11.8, 12.5]])
    rs = np.array([[0.31, 0.28], [1.12, 1.20], [1.25, 1.18]])
    theta = np.array([[0.05, 0.10, 0.20, 0.30, 8.0, 0.9], [0.10, 0.20, 0.30, 0.25, 10.5, 1.0]])
    S = los.LOSSamples(ds, rs, Ndraws=2)
    want = np.asarray(S(theta))
    want_tot, want_terms = S.terms(theta)
    assert want.shape == (2,) and np.all(np.isfinite(want)) and want_terms.shape == (2, 3)

    L = _lib.lib()
    th = np.ascontiguousarray(los._check_theta(theta, True, True)[0])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda")
    t_ds, t_rs, t_th = up(ds.T), up(rs.T), up(th)
    out = torch.empty(2, dtype=torch.float64, device="cuda")
    terms = torch.empty((2, 3), dtype=torch.float64, device="cuda")
    nbytes = int(L.brutus_los_workspace_bytes(3, 2))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    for t_terms in (None, terms):
        _lib.check(L.brutus_los_loglike(
            3, 2, t_ds.data_ptr(), t_rs.data_ptr(), None, 2, 1, t_th.data_ptr(), C.byref(S._p),
            out.data_ptr(), None if t_terms is None else t_terms.data_ptr(), ws.data_ptr(), nbytes,
            torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == want.tobytes()
    assert np.asarray(want_tot).tobytes() == want.tobytes()
    assert terms.cpu().numpy().tobytes() == want_terms.tobytes()


@pytest.mark.parametrize("bad", ("float32", "column view", "host array"))
def test_wrong_arguments_are_rejected_before_the_call(bad):
    from brutus_amd import _lib
    torch, x = _exp10_inputs()
    L = _lib.lib()
    arg = {"float32": lambda: x.to(torch.float32),
           "column view": lambda: torch.stack([x, x], dim=1)[:, 1],
           "host array": lambda: x.cpu().numpy()}[bad]()
    y = torch.full_like(x, -7.)
    with pytest.raises(C.ArgumentError, match="argument 1"):
        L.brutus_debug_exp10(arg, y, 64, None)
    with pytest.raises(C.ArgumentError, match="argument 2"):
        L.brutus_debug_exp10(x, arg, 64, None)
    torch.cuda.synchronize()
    assert torch.equal(y, torch.full_like(x, -7.))
