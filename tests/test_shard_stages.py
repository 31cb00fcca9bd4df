"""The stages of `parallel.fit_sharded` that need neither a process group nor a GPU: the
keyword table, the plan of who writes what, the runs of a resumed fit and the row packer.
(The protocol itself runs in test_parallel_gloo.py.)"""
import inspect
import os

import numpy as np
import pytest

from brutus_amd import h5io, parallel

NDRAWS = 3
ROWDT, POSITIONS = h5io.ResultsFile.row_dtype(NDRAWS, True)


def _res(row):
    """A 13-tuple as `_fit` yields it, every value a function of the row number."""
    val = np.arange(NDRAWS, dtype=np.float64) + 10. * row
    return (np.arange(NDRAWS) + row, val, val + .25, val + .5,
            np.full((NDRAWS, 3, 3), float(row)), 6 + row % 3, val + 1., float(row) + .125,
            1.5 * row, val + 2., val + 3., val + 4., val + 5.)


def _check_blocks(rows, chunk, expected):
    """Packs `rows`, compares `(start, n)` of the blocks with `expected` and checks what every
    case has to hold: each field of each entry, the input order, no shared memory."""
    blocks = list(parallel._pack_blocks(((r, _res(r)) for r in rows), chunk, ROWDT, POSITIONS))
    assert [(start, n) for start, n, _ in blocks] == expected
    packed = []
    for start, n, block in blocks:
        assert block.dtype == ROWDT and block.shape == (chunk,)
        for i in range(n):
            res = _res(start + i)
            for name, pos in POSITIONS:
                want = np.asarray(res[pos]).astype(ROWDT[name].base)
                assert np.array_equal(block[name][i], want), (start + i, name)
        packed.extend(range(start, start + n))
    assert packed == list(rows)
    for i, a in enumerate(blocks):
        for b in blocks[i + 1:]:
            assert not np.shares_memory(a[2], b[2])
    return blocks


@pytest.mark.parametrize("rows,chunk,expected", [
    ([0, 1, 2, 3, 4], 2, [(0, 2), (2, 2), (4, 1)]),
    ([2, 3, 4, 5], 8, [(2, 4)]),                  # two adjacent runs: consecutive rows continue a block
    ([1, 2, 7], 8, [(1, 2), (7, 1)]),             # the carried row opens the next block
    ([], 4, []),
    ([3, 4, 9], 1, [(3, 1), (4, 1), (9, 1)]),
])
def test_pack_blocks(rows, chunk, expected):
    _check_blocks(rows, chunk, expected)


def test_pack_blocks_takes_a_value_beyond_float32_without_raising():
    """`obj_log_evid` is float32 in the file; a float64 beyond its range becomes inf, as numpy
    casts it, whatever the caller's error state."""
    res = list(_res(0))
    res[7] = 1e300
    with np.errstate(over="raise"):
        blocks = list(parallel._pack_blocks([(0, tuple(res))], 4, ROWDT, POSITIONS))
    assert [(s, n) for s, n, _ in blocks] == [(0, 1)]
    assert np.isposinf(blocks[0][2]["obj_log_evid"][0])
    assert np.array_equal(blocks[0][2]["model_idx"][0], np.arange(NDRAWS))


def test_resume_runs():
    assert parallel._resume_runs(None, 3, 9) == [(3, 9)]
    assert parallel._resume_runs(None, 4, 4) == []
    mask = np.zeros(20, dtype=bool)
    mask[[0, 1, 2, 5, 6, 9, 12, 13, 14, 19]] = True
    assert parallel._resume_runs(mask, 0, 20) == [(0, 3), (5, 7), (9, 10), (12, 15), (19, 20)]
    # rows outside [lo, hi) are ignored, runs are cut at the shard's edges
    assert parallel._resume_runs(mask, 1, 14) == [(1, 3), (5, 7), (9, 10), (12, 14)]
    assert parallel._resume_runs(mask, 3, 5) == []
    for lo, hi in ((0, 20), (1, 14), (6, 13), (7, 7)):
        runs = parallel._resume_runs(mask, lo, hi)
        assert sum(b - a for a, b in runs) == mask[lo:hi].sum()
        assert all(mask[a:b].all() and lo <= a < b <= hi for a, b in runs)
        assert all(x[1] < y[0] for x, y in zip(runs[:-1], runs[1:]))       # maximal, in order
    assert parallel._resume_runs(np.zeros(20, dtype=bool), 0, 20) == []


# what `fit_sharded` passes to `_fit` by name
EXPLICIT = ("parallax", "parallax_err", "lnprior", "lngalprior", "lndustprior", "av_gauss",
            "wt_thresh", "data_coords", "Ndraws", "return_distreds", "seed0", "rstate_per_object",
            "lnprior_ext")
BOTH = ("cdf_thresh", "dustfile", "ltol_subthresh", "logl_initthresh")


def test_split_fit_kwargs():
    from brutus_amd.fitting import BruteForce
    setup_names = [k for k in inspect.signature(BruteForce._setup).parameters
                   if k not in ("self", "data", "data_err", "data_mask", "data_labels", "rstate")]
    assert len(setup_names) == 17
    kw = {k: object() for k in setup_names}
    kw.update(resume=1, Ndraws=11, save_dar_draws=False, running_io=False, lnprior_ext={"a": 1},
              verbose=True, rstate=object(), ltol=0.5, some_new_option=3)
    opts, skw, fkw = parallel._split_fit_kwargs(kw)
    assert opts == (True, 11, False, False, {"a": 1})
    assert opts._fields == ("resume", "Ndraws", "save_dar_draws", "running_io", "lnprior_ext")
    assert sorted(skw) == sorted(setup_names) and all(skw[k] is kw[k] for k in skw)
    assert not set(fkw) & set(EXPLICIT)
    for k in BOTH:
        assert skw[k] is kw[k] and fkw[k] is kw[k]
    for k in ("verbose", "rstate"):
        assert k not in skw and k not in fkw
    assert fkw["ltol"] == 0.5 and fkw["some_new_option"] == 3          # unknown: to `_fit`
    assert "ltol" not in skw and "some_new_option" not in skw
    assert sorted(fkw) == sorted(BOTH + ("ltol", "some_new_option", "logl_dim_prior"))
    # the table names nothing that `_setup` would not take
    assert {k for k, v in parallel._FIT_KWARGS.items() if v != "drop"} == set(setup_names)
    # defaults
    opts, skw, fkw = parallel._split_fit_kwargs({})
    assert opts == (False, 250, True, True, None) and skw == {} and fkw == {"logl_dim_prior": True}
    assert parallel._split_fit_kwargs({"logl_dim_prior": False})[2] == {"logl_dim_prior": False}


@pytest.mark.parametrize("share", [0., 1.])
def test_plan(tmp_path, share):
    save = os.path.join(str(tmp_path), "save")
    bounds = parallel.shard_bounds(10, 3, share)
    assert bounds == ([(0, 0), (0, 5), (5, 10)] if share == 0. else [(0, 4), (4, 7), (7, 10)])
    for r, (lo, hi) in enumerate(bounds):
        one = parallel._make_plan(r, bounds, "rank0", save, False)
        assert (one.lo, one.hi, one.per_rank, one.index_taken) == (lo, hi, False, False)
        assert one.owner == (r == 0)
        assert (one.my_path, one.my_rows, one.my_first) == (save + ".h5", 10, 0)
        per = parallel._make_plan(r, bounds, "per_rank", save, False)
        assert (per.lo, per.hi, per.per_rank, per.index_taken) == (lo, hi, True, False)
        assert per.owner == (hi > lo)
        assert (per.my_path, per.my_rows, per.my_first) == (save + ".r%02d.h5" % r, hi - lo, lo)
        assert per.index_path == one.index_path == save + ".h5"
        assert per.part_path(r) == per.my_path
        # the index names its parts by basename: they lie beside it
        assert per.index_parts() == [(a, b, os.path.basename(per.part_path(q)))
                                     for q, (a, b) in enumerate(bounds) if b > a]
        assert [p[2] for p in per.index_parts()] == ["save.r%02d.h5" % q for q in range(3)
                                                     if bounds[q][1] > bounds[q][0]]
    with pytest.raises(ValueError, match="writer must be 'rank0' or 'per_rank'"):
        parallel._make_plan(0, bounds, "rank1", save, False)


def test_plan_with_an_index_that_exists_already(tmp_path):
    """`writer="per_rank"`: rank 0 finds the index in its way before anything is fitted -- it opens
    nothing and `_open_results` hands back the OSError; a resume, the other ranks and the single
    writer (whose `ResultsFile` refuses by itself) are not concerned."""
    save = os.path.join(str(tmp_path), "save")
    open(save + ".h5", "w").close()
    bounds = parallel.shard_bounds(10, 3)
    plan = parallel._make_plan(0, bounds, "per_rank", save, False)
    assert plan.index_taken and not plan.owner
    out, err = parallel._open_results(plan, parallel._split_fit_kwargs({})[0], None)
    assert out is None and isinstance(err, OSError)
    assert str(err) == "fit_sharded: %s.h5 exists already" % save
    for args in ((0, bounds, "per_rank", save, True), (1, bounds, "per_rank", save, False),
                 (0, bounds, "rank0", save, False)):
        plan = parallel._make_plan(*args)
        assert plan.owner and not plan.index_taken
