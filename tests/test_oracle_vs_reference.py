"""The oracle against the upstream reference on fresh inputs: the reference's `loglike` and
`_fit` outputs for them are stored in tests/golden/oracle_fresh.npz (tools/gen_golden.py
`fresh`, run where the reference is importable)."""
import os

import numpy as np

from helpers import GOLDEN, galprior, relerr


def test_loglike_and_fit_fresh_inputs():
    from oracle import brutus_oracle as O
    from brutus_amd import synth
    z = np.load(os.path.join(GOLDEN, "oracle_fresh.npz"))
    models, labels, lmask = synth.make_mist_like_grid(int(z["grid_nmodel"]), int(z["grid_nfilt"]),
                                                      seed=int(z["grid_seed"]))
    st = {k: z[k] for k in ("flux", "err", "mask", "parallax", "parallax_err", "coords")}
    lnprior = O.static_lnprior(labels, lmask)
    assert np.array_equal(lnprior, z["lnprior"])
    for i in range(3):
        ref = [z["loglike_%d_%d" % (i, j)] for j in range(7)]
        got = O.loglike(st["flux"][i], st["err"][i], st["mask"][i], models,
                        parallax=st["parallax"][i],
                        parallax_err=st["parallax_err"][i], return_vals=True)
        assert len(got) == len(ref)
        for a, b in zip(ref, got):
            assert relerr(a, b) < 1e-10
        r = [z["fit_%d_%d" % (i, j)] for j in range(13)]
        o = O.fit_star(st["flux"][i], st["err"][i], st["mask"][i], models,
                       lnprior, labels, st["coords"][i], st["parallax"][i],
                       st["parallax_err"][i], np.random.RandomState(int(z["seed0"]) + i),
                       galprior, Nmc_prior=20, Ndraws=50)
        assert len(o) == len(r)
        assert np.array_equal(r[0], o[0])
        for a, b in zip(r[1:], o[1:]):
            assert relerr(a, b) < 1e-9
