"""GPU: the networks of `seds.Isochrone` (`k_iso_nn`) and `seds.SEDmaker` (`k_sed_nn_fit`) at
every compiled width of the first hidden layer.  The weights of a filter are staged into LDS
padded to 8, 16, 32 or 64 units (`nn_stage` in csrc/seds_common.hpp, and the same loops in
`k_sed_nn_fit`); the other GPU tests run width 16 in both paths and 64 in `SEDmaker` only.  Here
`h1` = 7, 8, 9, 31, 33, 64 gives the widths 8, 8, 16, 32, 64, 64, and the odd ones leave the
zero pad column that the pairwise second layer reads.  Against the numpy restatements, with the
bounds the project uses for this arithmetic against them: identical NaN patterns and selection,
magnitudes to 1e-9 absolute, parameters to 1e-9 relative, slopes to `SLOPE_TOL`."""
import numpy as np
import pytest

import iso_helpers as IH
import sed_helpers as SH
from test_gpu_sedmaker import MAG_TOL, PAR_RTOL, SLOPE_TOL, _plain, _relerr

pytestmark = pytest.mark.gpu

H1 = (7, 8, 9, 31, 33, 64)
EEP = np.linspace(202., 808., 300)          # (more than one workgroup of rows)


def _networks(h1):
    return IH.make_networks(2, h1, 3, 20 + h1)


@pytest.mark.parametrize("h1", H1)
def test_isochrone_at_every_width(h1):
    from brutus_amd import seds
    a = dict(zip(("feh", "afe", "loga", "eep", "pred_grid"), IH.make_table()))
    a.update(zip(("weights", "xmin", "xmax", "filters"), _networks(h1)))
    iso, host = seds.Isochrone.from_arrays(**a), IH.HostIsochrone(**a)
    worst = [0., 0.]
    for smf in (0., 0.5, 1.):
        kw = dict(IH.case_kwargs("young", smf), eep=EEP, smf=smf, return_dict=False)
        got, want = iso.get_seds(**kw), host.get_seds(**kw)
        assert np.isfinite(want[0]).any() and np.isnan(want[0]).any()
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)), (smf, k)
            fin = np.isfinite(w)
            assert np.array_equal(np.isfinite(g), fin), (smf, k)
            if fin.any():
                err = float(np.max(np.abs(g[fin] - w[fin]))) if k == 0 else _relerr(g, w)
                worst[k > 0] = max(worst[k > 0], err)
    print("Isochrone h1=%d: worst errors: magnitudes %.3g, parameters (relative) %.3g"
          % (h1, worst[0], worst[1]))
    assert worst[0] < MAG_TOL and worst[1] < PAR_RTOL


@pytest.fixture(scope="module")
def tracks():
    """The tracks of grid A and the secondaries' EEPs of its models from the host's solve (they
    do not depend on the networks): no width below involves a solve."""
    labels, output = SH.make_tracks(two_afe=True)
    w, xmin, xmax, filters = _networks(H1[0])
    host = SH.HostSEDmaker(labels, output, w, xmin, xmax, filters)
    return labels, output, host.make_grid(**SH.GRID_A)[4]


@pytest.mark.parametrize("h1", H1)
def test_make_grid_at_every_width(tracks, h1):
    from brutus_amd import seds
    labels, output, eep2 = tracks
    w, xmin, xmax, filters = _networks(h1)
    sm = seds.SEDmaker.from_arrays(labels, output, w, xmin, xmax, filters)
    host = SH.HostSEDmaker(labels, output, w, xmin, xmax, filters)
    sm.make_grid(eep2=eep2, verbose=False, **SH.GRID_A)
    hlab, hsed, hpar, hsel, _ = host.make_grid(eep2=eep2, **SH.GRID_A)
    lab, sed, par, sel = _plain(sm)
    assert len(lab) == 1512 and np.array_equal(lab, hlab)
    assert np.array_equal(sel, hsel) and 100 < sel.sum() < 1512
    assert (lab[sel][:, 4] > 0.).any()                              # (binaries among them)
    assert np.array_equal(np.isnan(sed), np.isnan(hsed)) and np.isnan(sed[~sel]).all()
    perr = _relerr(par, hpar)
    merr = float(np.max(np.abs(sed[sel][..., 0] - hsed[sel][..., 0])))
    serr = float(np.max(np.abs(sed[sel][..., 1:] - hsed[sel][..., 1:])))
    print("SEDmaker h1=%d: worst errors: magnitudes %.3g, parameters (relative) %.3g, slopes %.3g"
          % (h1, merr, perr, serr))
    assert merr < MAG_TOL and perr < PAR_RTOL and serr < SLOPE_TOL
