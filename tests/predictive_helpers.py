"""What tests/test_predictive_host.py, tests/test_gpu_predictive.py and the `post_predictive` case
of tools/gen_golden.py share: the fixture's shapes and the scale a column's tolerance is a
fraction of.  The draw counts, the margin to the knots and the knots themselves are those of
summary_helpers."""
import os

import numpy as np

from summary_helpers import MARGIN, NFLOAT, NSAMPS, knots, margin, nobj_of  # noqa: F401

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "post_predictive.npz")
#: the grid: synth.make_mist_like_grid(NMODEL, NFILT, seed=GRID_SEED), float32
NMODEL, NFILT, GRID_SEED = 500, 8, 7
Q = (0., 0.025, 0.16, 0.5, 0.84, 0.975, 1.)
#: draw counts whose `seds` arrays the fixture keeps (the minimum, past a wave, fit()'s default)
SEDS_NSAMPS = (2, 65, 250)
SPACES = ("mag", "flux")         # flux = False, True


def scale(seds, flux):
    """The scale of every band's column of `seds (..., Nsamps, Nfilt)`: max(1, largest finite
    |x|) in magnitude space, the largest finite |x| in flux space -- fluxes are around 1e-8, the
    max(1, .) form would hide everything."""
    with np.errstate(all="ignore"):
        a = np.where(np.isfinite(seds), np.abs(seds), 0.).max(axis=-2)
    return a if flux else np.maximum(1., a)
