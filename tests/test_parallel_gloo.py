"""CPU, world_size 2, gloo: the star-sharding plumbing of brutus_amd.parallel
(`fit_sharded`; bench.py's N > 1 path does not go through it).  The HIP engine itself cannot run
here, so `_fit` is replaced by a deterministic stand-in; what is under test is
the partition, the rank-ordered gather, the per-object seeding and the HDF5
assembly."""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_shard_range_partitions_everything():
    from brutus_amd.parallel import shard_range
    for n in (0, 1, 7, 10, 1000003):
        for world in (1, 2, 3, 8):
            edges = [shard_range(n, r, world) for r in range(world)]
            assert edges[0][0] == 0 and edges[-1][1] == n
            for (a, b), (c, d) in zip(edges[:-1], edges[1:]):
                assert b == c and a <= b
            sizes = [b - a for a, b in edges]
            assert max(sizes) - min(sizes) <= 1


def _worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from brutus_amd import fitting, parallel, synth
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port,
                            rank=rank, world_size=world)
    models, labels, lmask = synth.make_grid(64, 6, seed=1)
    st = synth.make_stars(models, 11, seed=2)

    class Stub(fitting.BruteForce):
        def _fit(self, data, data_err, data_mask, parallax=None, Ndraws=250,
                 seed0=None, return_distreds=True, rstate_per_object=None, **kw):
            for i in range(data.shape[0]):
                rs = np.random.RandomState(seed0 + i)
                idx = rs.randint(0, 64, size=Ndraws)
                val = np.full(Ndraws, float(np.sum(data[i])))
                yield (idx, val, val, val, np.zeros((Ndraws, 3, 3)), 6, val,
                       float(rs.uniform()), 1.5, val, val, val, val)

    bf = Stub(models, labels, lmask)
    # broadcast_array: only rank 0 knows the payload
    arr = parallel.broadcast_array(np.arange(12.).reshape(3, 4) if rank == 0 else None)
    assert np.array_equal(arr, np.arange(12.).reshape(3, 4))
    lab = np.zeros(11, dtype=[("id", "i8")])
    lab["id"] = np.arange(11)
    n = parallel.fit_sharded(bf, st["flux"], st["err"], st["mask"], lab,
                             os.path.join(tmp, "out_w%d" % world), seed0=100,
                             Ndraws=5, lngalprior=lambda *a, **k: 0.,
                             parallax=st["parallax"],
                             parallax_err=st["parallax_err"],
                             data_coords=st["coords"])
    lo, hi = parallel.shard_range(11, rank, world)
    assert n == hi - lo
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [1, 2])
def test_fit_sharded_gloo(tmp_path, world):
    import torch.multiprocessing as mp
    from brutus_amd import h5io
    port = _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    path = os.path.join(str(tmp_path), "out_w%d.h5" % world)
    idx = h5io.read_dataset(path, "model_idx")
    assert idx.shape == (11, 5) and idx.dtype == np.int32
    # object i always draws from RandomState(100 + i), whatever the sharding
    for i in range(11):
        rs = np.random.RandomState(100 + i)
        assert np.array_equal(idx[i], rs.randint(0, 64, size=5))
    assert np.array_equal(h5io.read_dataset(path, "labels")["id"], np.arange(11))
    assert np.all(h5io.read_dataset(path, "obj_Nbands") == 6)


def _worker_big(rank, world, port, tmp, ndata, chunk):
    """10^5 objects through the chunked hand-off: rows are handed to rank 0 in bounded
    pieces, so no rank's resident set may grow with the catalogue."""
    sys.path.insert(0, ROOT)
    import resource
    import torch.distributed as dist
    from brutus_amd import fitting, parallel, synth
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port,
                            rank=rank, world_size=world)
    models, labels, lmask = synth.make_grid(64, 6, seed=1)
    rng = np.random.RandomState(5)
    flux = rng.uniform(1e-9, 1e-8, size=(ndata, 6))
    err = 0.05 * flux
    mask = np.ones((ndata, 6), dtype=bool)
    ext = {"feh": np.stack([np.arange(ndata, dtype=float), np.ones(ndata)], axis=1)}
    seen = {"max_live": 0}

    class Stub(fitting.BruteForce):
        def _fit(self, data, data_err, data_mask, Ndraws=250, seed0=None,
                 lnprior_ext=None, **kw):
            assert lnprior_ext["feh"].shape[0] == data.shape[0]      # sliced to the shard
            for i in range(data.shape[0]):
                val = np.full(Ndraws, float(seed0 + i))
                # obj_chi2min carries the object's OWN external constraint
                yield (np.full(Ndraws, (seed0 + i) % 64), val, val, val,
                       np.zeros((Ndraws, 3, 3)), 6, val, float(seed0 + i),
                       float(lnprior_ext["feh"][i, 0]), val, val, val, val)

    bf = Stub(models, labels, lmask)
    lab = np.zeros(ndata, dtype=[("id", "i8")])
    lab["id"] = np.arange(ndata)
    import time
    rss0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    t0 = time.time()
    n = parallel.fit_sharded(bf, flux, err, mask, lab, os.path.join(tmp, "big_w%d" % world),
                             seed0=0, Ndraws=8, chunk=chunk, lngalprior=lambda *a, **k: 0.,
                             data_coords=np.zeros((ndata, 2)), lnprior_ext=ext)
    dt = time.time() - t0
    rss1 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    lo, hi = parallel.shard_range(ndata, rank, world)
    assert n == hi - lo
    # one finished row here is ~1.6 KB (Ndraws = 8); holding a whole shard of 5 x 10^4
    # rows (the old list(...) + gather_object of everything) costs > 150 MB on rank 0.
    # The bounded hand-off keeps the growth to the staging of `world * chunk` rows.
    grew_mb = (rss1 - rss0) / 1024.
    with open(os.path.join(tmp, "rss_w%d_%d.txt" % (world, rank)), "w") as f:
        f.write("%.1f %.3f" % (grew_mb, dt))
    dist.destroy_process_group()


def test_fit_sharded_streams_1e5_rows_with_bounded_memory(tmp_path):
    """10^5 stub rows through the packed-block hand-off (gloo side group, no pickling) and
    the asynchronous writer: every row at its place, resident sets bounded, >= 30 k rows/s,
    and the file BYTE-IDENTICAL to the one a single process writes."""
    import filecmp
    import torch.multiprocessing as mp
    from brutus_amd import h5io
    ndata = 100000
    for world in (1, 2):
        port = _free_port()
        mp.spawn(_worker_big, args=(world, port, str(tmp_path), ndata, 512), nprocs=world, join=True)
    path = os.path.join(str(tmp_path), "big_w2.h5")
    evid = h5io.read_dataset(path, "obj_log_evid")
    chi2 = h5io.read_dataset(path, "obj_chi2min")
    idx = h5io.read_dataset(path, "model_idx")
    assert evid.shape == (ndata,) and idx.shape == (ndata, 8)
    # every row at its catalogue position, on both sides of the shard boundary
    assert np.array_equal(evid.astype(np.int64), np.arange(ndata))
    assert np.array_equal(idx[:, 0], np.arange(ndata) % 64)
    # lnprior_ext reached each rank sliced to its own objects (rank 1 used to
    # see the constraints of objects 0..n)
    assert np.array_equal(chi2.astype(np.int64), np.arange(ndata))
    assert filecmp.cmp(path, os.path.join(str(tmp_path), "big_w1.h5"), shallow=False)
    for world in (1, 2):
        for r in range(world):
            grew, dt = (float(x) for x in
                        open(os.path.join(str(tmp_path), "rss_w%d_%d.txt" % (world, r))).read().split())
            assert grew < 80., (world, r, grew)
            assert ndata / dt > 30000., (world, r, ndata / dt)


def _worker_balance(rank, world, port, tmp, ndata, fail_rank):
    """A stand-in fit that takes 0.4 ms per object (sleeping, like a rank waiting for its GPU)."""
    sys.path.insert(0, ROOT)
    import time
    import torch.distributed as dist
    from brutus_amd import fitting, parallel, synth
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port,
                            rank=rank, world_size=world)
    models, labels, lmask = synth.make_grid(64, 6, seed=1)
    rng = np.random.RandomState(5)
    flux = rng.uniform(1e-9, 1e-8, size=(ndata, 6))

    class Stub(fitting.BruteForce):
        def _fit(self, data, data_err, data_mask, Ndraws=250, seed0=None, **kw):
            for i in range(data.shape[0]):
                time.sleep(4e-4)
                if rank == fail_rank and i == 100:
                    raise FloatingPointError("star %d of rank %d" % (i, rank))
                val = np.full(Ndraws, float(seed0 + i))
                yield (np.full(Ndraws, (seed0 + i) % 64), val, val, val,
                       np.zeros((Ndraws, 3, 3)), 6, val, float(seed0 + i), 1., val, val, val, val)

    bf = Stub(models, labels, lmask)
    msg = "ok"
    # what the same number of sleeps costs on this box right now, all ranks sleeping at once
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(300):
        time.sleep(4e-4)
    base = (time.perf_counter() - t0) * (ndata // world) / 300.
    try:
        parallel.fit_sharded(bf, flux, 0.05 * flux, np.ones((ndata, 6), dtype=bool), None,
                             os.path.join(tmp, "bal"), seed0=0, Ndraws=8, chunk=64,
                             lngalprior=lambda *a, **k: 0., data_coords=np.zeros((ndata, 2)))
        st = parallel.fit_sharded.last_stats
        msg = "ok %.4f %.4f %.4f" % (st["fit_s"], st["total_s"], base)
    except FloatingPointError as e:
        msg = "own %s" % e
    except RuntimeError as e:
        msg = "remote %s" % e
    with open(os.path.join(tmp, "bal_%d.txt" % rank), "w") as f:
        f.write(msg)
    dist.destroy_process_group()


def test_fit_sharded_eight_ranks_rank0_is_not_the_straggler(tmp_path):
    """World size 8 on CPU stand-ins: rank 0 fits an equal shard AND receives, unpacks and
    writes everybody's rows (in its hand-off thread); its fit must end with the others'
    (within 25 %), and no rank's fit may be stretched by waiting for another rank's rounds
    (round 3's lock-step gather put rank 0's extra work into every rank's loop)."""
    import torch.multiprocessing as mp
    from brutus_amd import h5io
    world, ndata = 8, 8 * 1500
    mp.spawn(_worker_balance, args=(world, _free_port(), str(tmp_path), ndata, -1), nprocs=world, join=True)
    res = [open(os.path.join(str(tmp_path), "bal_%d.txt" % r)).read().split() for r in range(world)]
    assert all(x[0] == "ok" for x in res), res
    fit = np.array([float(x[1]) for x in res])
    base = np.array([float(x[3]) for x in res])             # the shard's sleeps alone, same box, same moment
    others = np.median(fit[1:])
    evid = h5io.read_dataset(os.path.join(str(tmp_path), "bal.h5"), "obj_log_evid")
    assert np.array_equal(evid.astype(np.int64), np.arange(ndata))
    if np.median(base) > 1500 * 4e-4 * 2.0:
        pytest.skip("the box is too loaded for a timing statement (a 0.4 ms sleep takes %.2f ms)"
                    % (np.median(base) / 1500 * 1e3))
    assert fit.max() <= 1.6 * np.median(base) + 0.2, (fit, base)     # the fit = its own sleeps
    # (sixteen threads on the eight cores of the CPU box: a sleep of 0.4 ms takes 0.6-0.7, and
    # the ranks differ by 10-15 % on their own; lock-step rounds would cost every rank rank 0's
    # unpacking and writing of ALL rows on top, i.e. a factor, not a fraction)
    assert fit[0] <= 1.35 * others + 0.1, fit               # rank 0 is not the straggler


def test_fit_sharded_failure_on_one_rank_stops_all(tmp_path):
    """A fit that raises on rank 2 of 4: that rank re-raises its own error, every other rank
    raises a RuntimeError naming it, and nobody is left waiting in a collective (the spawn
    would hang; round 3's gather loop did)."""
    import torch.multiprocessing as mp
    world, ndata = 4, 4 * 800
    mp.spawn(_worker_balance, args=(world, _free_port(), str(tmp_path), ndata, 2), nprocs=world, join=True)
    res = [open(os.path.join(str(tmp_path), "bal_%d.txt" % r)).read() for r in range(world)]
    assert res[2].startswith("own star 100 of rank 2"), res
    for r in (0, 1, 3):
        assert res[r].startswith("remote") and "rank(s) 2" in res[r], res


def test_shard_bounds_with_a_lighter_rank0():
    from brutus_amd.parallel import shard_bounds, shard_range
    assert shard_bounds(100, 4) == [shard_range(100, r, 4) for r in range(4)]
    for share in (0., 0.5):
        b = shard_bounds(1000, 8, share)
        assert b[0][0] == 0 and b[-1][1] == 1000 and all(x[1] == y[0] for x, y in zip(b[:-1], b[1:]))
        sizes = [y - x for x, y in b]
        assert abs(sizes[0] - share * sizes[1]) <= 1 and max(sizes[1:]) - min(sizes[1:]) <= 1


def _stub_class(fail_at=None):
    """A deterministic stand-in for the GPU fit: row i depends on `seed0 + i` and the data only."""
    sys.path.insert(0, ROOT)
    from brutus_amd import fitting

    class Stub(fitting.BruteForce):
        def _fit(self, data, data_err, data_mask, Ndraws=250, seed0=None, **kw):
            for i in range(data.shape[0]):
                if fail_at is not None and seed0 + i == fail_at:
                    raise FloatingPointError("object %d" % (seed0 + i))
                rs = np.random.RandomState(seed0 + i)
                val = rs.uniform(size=Ndraws) + float(np.sum(data[i])) * 1e8
                yield (rs.randint(0, 64, size=Ndraws), val, val + 1., val + 2.,
                       rs.uniform(size=(Ndraws, 3, 3)), 6, val + 3., float(rs.uniform()), 1.5,
                       val + 4., val + 5., val + 6., val + 7.)
    return Stub


def _worker_resume(rank, world, port, tmp, name, fail_at, resume, writer="rank0"):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from brutus_amd import parallel, synth
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port,
                            rank=rank, world_size=world)
    models, labels, lmask = synth.make_grid(64, 6, seed=1)
    ndata = 301
    rng = np.random.RandomState(5)
    flux = rng.uniform(1e-9, 1e-8, size=(ndata, 6))
    bf = _stub_class(fail_at)(models, labels, lmask)
    msg = "ok"
    try:
        n = parallel.fit_sharded(bf, flux, 0.05 * flux, np.ones((ndata, 6), dtype=bool), None,
                                 os.path.join(tmp, name), seed0=1000, Ndraws=7, chunk=16,
                                 lngalprior=lambda *a, **k: 0., data_coords=np.zeros((ndata, 2)),
                                 resume=resume, writer=writer)
        msg = "ok %d" % n
    except FloatingPointError as e:
        msg = "own %s" % e
    except OSError as e:
        msg = "own OSError %s" % e
    except RuntimeError as e:
        msg = "remote %s" % e
    with open(os.path.join(tmp, "%s_%d.txt" % (name, rank)), "w") as f:
        f.write(msg)
    dist.destroy_process_group()


def test_fit_sharded_resume_completes_an_interrupted_file(tmp_path):
    """World size 2: the fit of object 1230 (rank 1's shard) raises, every rank stops, the
    file keeps the sentinel in the rows that never arrived.  `resume=True` -- with THREE ranks
    this time -- fits exactly those rows and the file equals an uninterrupted single-rank
    run's, dataset by dataset (reference fitting.py:1635: `model_idx == -99` marks a row as
    not yet fitted)."""
    import torch.multiprocessing as mp
    from brutus_amd import h5io
    tmp = str(tmp_path)
    mp.spawn(_worker_resume, args=(1, _free_port(), tmp, "full", None, False), nprocs=1, join=True)
    mp.spawn(_worker_resume, args=(2, _free_port(), tmp, "part", 1230, False), nprocs=2, join=True)
    res = [open(os.path.join(tmp, "part_%d.txt" % r)).read() for r in range(2)]
    assert res[1].startswith("own object 1230") and res[0].startswith("remote"), res
    idx = h5io.read_dataset(os.path.join(tmp, "part.h5"), "model_idx")
    missing = np.flatnonzero(idx[:, 0] == -99)
    assert 0 < missing.size < 301 and 230 in missing
    mp.spawn(_worker_resume, args=(3, _free_port(), tmp, "part", None, True), nprocs=3, join=True)
    res = [open(os.path.join(tmp, "part_%d.txt" % r)).read().split() for r in range(3)]
    assert all(x[0] == "ok" for x in res), res
    assert sum(int(x[1]) for x in res) == missing.size          # only the unfinished rows were fitted
    names = h5io.list_datasets(os.path.join(tmp, "full.h5"))
    assert "model_idx" in names and len(names) >= 12
    for k in names:
        a = h5io.read_dataset(os.path.join(tmp, "full.h5"), k)
        b = h5io.read_dataset(os.path.join(tmp, "part.h5"), k)
        assert a.dtype == b.dtype and np.array_equal(a, b), k


def _worker_close_fails(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from brutus_amd import h5io, parallel, synth
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port,
                            rank=rank, world_size=world)
    models, labels, lmask = synth.make_grid(64, 6, seed=1)
    ndata = 120
    flux = np.random.RandomState(5).uniform(1e-9, 1e-8, size=(ndata, 6))
    bf = _stub_class()(models, labels, lmask)
    real_close = h5io.ResultsFile.close

    def close(self):                      # the writer's last blocks hit a full disk
        real_close(self)
        if not getattr(self, "_failed_once", False):
            self._failed_once = True
            raise OSError("No space left on device")
    h5io.ResultsFile.close = close
    try:
        parallel.fit_sharded(bf, flux, 0.05 * flux, np.ones((ndata, 6), dtype=bool), None,
                             os.path.join(tmp, "cf"), seed0=0, Ndraws=5, chunk=16,
                             lngalprior=lambda *a, **k: 0., data_coords=np.zeros((ndata, 2)))
        msg = "ok"
    except OSError as e:
        msg = "own %s" % e
    except RuntimeError as e:
        msg = "remote %s" % e
    with open(os.path.join(tmp, "cf_%d.txt" % rank), "w") as f:
        f.write(msg)
    dist.destroy_process_group()


def test_fit_sharded_writer_failure_at_the_very_end_reaches_every_rank(tmp_path):
    """The writer is asynchronous: an error in its last blocks only shows when rank 0 flushes
    and closes the file -- after every rank has reported "done".  The closing round of the
    hand-off protocol carries it: rank 0 raises the OSError, the others a RuntimeError, and
    nobody waits in the final barrier (the spawn would hang)."""
    import torch.multiprocessing as mp
    mp.spawn(_worker_close_fails, args=(3, _free_port(), str(tmp_path)), nprocs=3, join=True)
    res = [open(os.path.join(str(tmp_path), "cf_%d.txt" % r)).read() for r in range(3)]
    assert res[0].startswith("own No space left"), res
    assert all(r.startswith("remote") and "rank 0" in r for r in res[1:]), res


def _worker_per_rank(rank, world, port, tmp, writer, resume_rows):
    """`fit_sharded(writer=...)` with a deterministic stand-in for `_fit`; `resume_rows`: first
    pass fits everything but dies... no: rows to blank out again before a resume pass."""
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from brutus_amd import fitting, parallel, synth
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port,
                            rank=rank, world_size=world)
    models, labels, lmask = synth.make_grid(64, 6, seed=1)
    st = synth.make_stars(models, 23, seed=2)

    class Stub(fitting.BruteForce):
        def _fit(self, data, data_err, data_mask, parallax=None, Ndraws=250,
                 seed0=None, return_distreds=True, rstate_per_object=None, **kw):
            for i in range(data.shape[0]):
                rs = np.random.RandomState(seed0 + i)
                idx = rs.randint(0, 64, size=Ndraws)
                val = rs.uniform(size=Ndraws)
                cov = rs.uniform(size=(Ndraws, 3, 3))
                yield (idx, val, 2. * val, 3. * val, cov, 6, val - 1.,
                       float(rs.uniform()), float(np.sum(data[i])), val, val + 1., val + 2., val + 3.)

    bf = Stub(models, labels, lmask)
    lab = np.zeros(23, dtype=[("id", "i8"), ("name", "S6")])
    lab["id"] = np.arange(23)
    lab["name"] = [b"s%04d" % i for i in range(23)]
    n = parallel.fit_sharded(bf, st["flux"], st["err"], st["mask"], lab,
                             os.path.join(tmp, "%s_w%d" % (writer, world)), seed0=100,
                             Ndraws=5, chunk=4, lngalprior=lambda *a, **k: 0.,
                             parallax=st["parallax"], parallax_err=st["parallax_err"],
                             data_coords=st["coords"], writer=writer)
    lo, hi = parallel.shard_range(23, rank, world)
    assert n == hi - lo
    assert parallel.fit_sharded.last_stats["writer"] == writer
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_per_rank_writer_index_equals_the_single_writer_file(tmp_path, world):
    """`writer="per_rank"`: every rank writes `{save_file}.rNN.h5`, rank 0 an index of virtual
    datasets -- read through the index, every dataset equals the file one writer on rank 0
    produces, for 1 - 8 ranks (8 ranks on 23 objects: shards of 2 - 3 rows), and
    `h5io.materialize` turns the index into one plain file with the same content."""
    import torch.multiprocessing as mp
    from brutus_amd import h5io
    for writer in ("rank0", "per_rank"):
        mp.spawn(_worker_per_rank, args=(world, _free_port(), str(tmp_path), writer, None),
                 nprocs=world, join=True)
    one = os.path.join(str(tmp_path), "rank0_w%d.h5" % world)
    idx = os.path.join(str(tmp_path), "per_rank_w%d.h5" % world)
    names = sorted(h5io.list_datasets(one))
    assert names == sorted(h5io.list_datasets(idx)) and len(names) == 14
    parts = [f for f in os.listdir(str(tmp_path)) if f.startswith("per_rank_w%d.r" % world)]
    assert len(parts) == world
    here = os.getcwd()
    os.chdir("/")                        # (the index finds its parts relative to ITSELF)
    try:
        for k in names:
            a, b = h5io.read_dataset(one, k), h5io.read_dataset(idx, k)
            assert a.dtype == b.dtype and a.shape == b.shape, k
            assert np.array_equal(a, b), k
        flat = os.path.join(str(tmp_path), "flat_w%d.h5" % world)
        h5io.materialize(idx, flat)
        for k in names:
            assert np.array_equal(h5io.read_dataset(one, k), h5io.read_dataset(flat, k)), k
    finally:
        os.chdir(here)


def test_fit_sharded_resume_with_per_rank_parts(tmp_path):
    """`writer="per_rank"`, three ranks: object 1230 (rank 2's shard) raises, everybody stops, no
    index is written.  `resume=True` with the same three ranks re-opens every part, fits the rows
    that still hold the sentinel and writes the index: equal to an uninterrupted single-writer run."""
    import torch.multiprocessing as mp
    from brutus_amd import h5io
    tmp = str(tmp_path)
    mp.spawn(_worker_resume, args=(1, _free_port(), tmp, "full", None, False), nprocs=1, join=True)
    mp.spawn(_worker_resume, args=(3, _free_port(), tmp, "pp", 1230, False, "per_rank"), nprocs=3, join=True)
    res = [open(os.path.join(tmp, "pp_%d.txt" % r)).read() for r in range(3)]
    assert res[2].startswith("own object 1230") and all(r.startswith("remote") for r in res[:2]), res
    assert not os.path.exists(os.path.join(tmp, "pp.h5"))
    mp.spawn(_worker_resume, args=(3, _free_port(), tmp, "pp", None, True, "per_rank"), nprocs=3, join=True)
    res = [open(os.path.join(tmp, "pp_%d.txt" % r)).read().split() for r in range(3)]
    assert all(x[0] == "ok" for x in res), res
    assert 0 < sum(int(x[1]) for x in res) < 301            # only the unfinished rows were fitted
    for k in h5io.list_datasets(os.path.join(tmp, "full.h5")):
        a = h5io.read_dataset(os.path.join(tmp, "full.h5"), k)
        b = h5io.read_dataset(os.path.join(tmp, "pp.h5"), k)
        assert a.dtype == b.dtype and np.array_equal(a, b), k


def test_fit_sharded_file_that_cannot_be_created_stops_every_rank(tmp_path):
    """The results file exists already (`"w-"`, reference fitting.py:1632): rank 0 raises its
    OSError and the other ranks a RuntimeError naming it -- before anybody enters the hand-off
    protocol (they used to wait for rank 0 in its first round); same with per-rank parts when
    one rank's part exists."""
    import torch.multiprocessing as mp
    tmp = str(tmp_path)
    open(os.path.join(tmp, "ex.h5"), "w").close()
    mp.spawn(_worker_resume, args=(3, _free_port(), tmp, "ex", None, False), nprocs=3, join=True)
    res = [open(os.path.join(tmp, "ex_%d.txt" % r)).read() for r in range(3)]
    assert res[0].startswith("own OSError"), res
    assert all(r.startswith("remote") and "rank(s) 0" in r for r in res[1:]), res
    open(os.path.join(tmp, "ez.h5"), "w").close()            # per-rank parts: the INDEX exists already
    mp.spawn(_worker_resume, args=(2, _free_port(), tmp, "ez", None, False, "per_rank"), nprocs=2, join=True)
    res = [open(os.path.join(tmp, "ez_%d.txt" % r)).read() for r in range(2)]
    assert res[0].startswith("own OSError") and res[1].startswith("remote"), res
    assert not [f for f in os.listdir(tmp) if f.startswith("ez.r")]      # nothing was fitted, no part left behind
    open(os.path.join(tmp, "ey.r01.h5"), "w").close()
    mp.spawn(_worker_resume, args=(3, _free_port(), tmp, "ey", None, False, "per_rank"), nprocs=3, join=True)
    res = [open(os.path.join(tmp, "ey_%d.txt" % r)).read() for r in range(3)]
    assert res[1].startswith("own OSError"), res
    assert all(res[r].startswith("remote") and "rank(s) 1" in res[r] for r in (0, 2)), res
