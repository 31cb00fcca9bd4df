"""Multi-GPU plumbing: one process per GPU, `torch.distributed` (backend "nccl"
= RCCL over xGMI on ROCm; "gloo" in the CPU tests).

The path shards by stars: objects are independent (the reference's star loop,
fitting.py:1980, has no cross-star coupling except its RNG stream), so each
rank fits a contiguous range of the catalogue and there is NO collective on the
data path.  The only collective is the one-off broadcast of the model grid in
kernel layout (108 MB at 750k x 12) and of the static prior vector.
"""
import collections
import functools
import os
import queue
import threading
import time

import numpy as np

__all__ = ["shard_range", "shard_bounds", "broadcast_grid", "broadcast_array", "fit_sharded"]


def shard_range(n, rank, world):
    """Contiguous [lo, hi) of `n` objects for `rank` (keeps output row order;
    sizes differ by at most one)."""
    base, rem = divmod(int(n), int(world))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def shard_bounds(n, world, rank0_share=1.0):
    """[lo, hi) of every rank.  `rank0_share` < 1 gives rank 0 -- which also receives and
    writes everybody's rows -- that fraction of an equal share (0: rank 0 only writes);
    1.0 is `shard_range`."""
    n, world = int(n), int(world)
    if world == 1 or rank0_share >= 1.:
        return [shard_range(n, r, world) for r in range(world)]
    n0 = int(round(max(0., float(rank0_share)) * n / (world - 1 + max(0., float(rank0_share)))))
    rest = [shard_range(n - n0, r, world - 1) for r in range(world - 1)]
    return [(0, n0)] + [(n0 + a, n0 + b) for a, b in rest]


def broadcast_grid(grid, nmodel, nfilt, device, src=0):
    """Broadcast the SoA grid tensor from `src`; returns a DeviceGrid on every
    rank.  `grid` is the source rank's DeviceGrid (None elsewhere)."""
    import torch
    import torch.distributed as dist
    from . import _lib
    from .fitting import DeviceGrid
    nbytes = _lib.lib().brutus_grid_soa_bytes(nmodel, nfilt)
    if grid is not None:
        soa = grid.soa
    else:
        soa = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
    dist.broadcast(soa, src=src)
    return DeviceGrid.from_soa(soa, nmodel, nfilt)


def broadcast_array(arr, src=0, device=None):
    """Broadcast a numpy array (shape/dtype known on `src` only)."""
    import torch
    import torch.distributed as dist
    rank = dist.get_rank()
    meta = [None]
    if rank == src:
        arr = np.ascontiguousarray(arr)
        meta = [(arr.shape, arr.dtype.str)]
    dist.broadcast_object_list(meta, src=src)
    shape, dt = meta[0]
    if rank != src:
        arr = np.empty(shape, dtype=np.dtype(dt))
    t = torch.from_numpy(arr.view(np.uint8).reshape(-1))
    if device is not None:
        t = t.to(device)
    dist.broadcast(t, src=src)
    if device is not None:
        arr = t.cpu().numpy().view(np.dtype(dt)).reshape(shape)
    return arr


# Where a `BruteForce.fit` keyword goes in `fit_sharded`.  "setup": to `_setup` alone, which hands
# back what `_fit` needs of it and `fit_sharded` passes that on by name; "both": to `_setup` and to
# `_fit`; "drop": to neither (`_fit` gets a stream per object instead of `rstate`).  The driver's
# own options are `_Options`; a keyword that is in neither goes to `_fit` ("fit").
_FIT_KWARGS = {
    "phot_offsets": "setup", "parallax": "setup", "parallax_err": "setup", "av_gauss": "setup",
    "lnprior": "setup", "wt_thresh": "setup", "apply_agewt": "setup", "apply_grad": "setup",
    "lngalprior": "setup", "lndustprior": "setup", "data_coords": "setup", "mag_max": "setup",
    "merr_max": "setup",
    "cdf_thresh": "both", "dustfile": "both", "ltol_subthresh": "both", "logl_initthresh": "both",
    "verbose": "drop", "rstate": "drop"}

_Options = collections.namedtuple("_Options", "resume Ndraws save_dar_draws running_io lnprior_ext")


def _split_fit_kwargs(fit_kwargs):
    """`(options, _setup keywords, _fit keywords)` of `fit_sharded`'s `**fit_kwargs`."""
    kw = dict(fit_kwargs)
    opts = _Options(bool(kw.pop("resume", False)), kw.pop("Ndraws", 250),
                    kw.pop("save_dar_draws", True), kw.pop("running_io", True),
                    kw.pop("lnprior_ext", None))
    skw = {k: v for k, v in kw.items() if _FIT_KWARGS.get(k) in ("setup", "both")}
    fkw = {k: v for k, v in kw.items() if _FIT_KWARGS.get(k, "fit") in ("both", "fit")}
    fkw.setdefault("logl_dim_prior", True)
    return opts, skw, fkw


class _Plan(collections.namedtuple(
        "_Plan", "rank bounds save_file lo hi per_rank owner my_path my_rows my_first index_path "
                 "index_taken")):
    """Who writes what: one file on rank 0 (rows arrive over the side group), or a part per rank
    with rows and an index on rank 0.  `owner`: this rank opens `my_path` (`my_rows` rows, the
    first one catalogue row `my_first`)."""
    __slots__ = ()

    def part_path(self, r):
        return _part_path(self.save_file, r)

    def index_parts(self):
        """`(lo, hi, file name beside the index)` of every part, for `h5io.write_virtual_index`."""
        return [(a, b, os.path.basename(self.part_path(r)))
                for r, (a, b) in enumerate(self.bounds) if b > a]


def _part_path(save_file, r):
    return "{0}.r{1:02d}.h5".format(save_file, r)


def _make_plan(rank, bounds, writer, save_file, resume):
    """The `_Plan` of `rank`; `bounds` are every rank's `[lo, hi)`."""
    if writer not in ("rank0", "per_rank"):
        raise ValueError("fit_sharded: writer must be 'rank0' or 'per_rank'")
    per_rank = writer == "per_rank"
    lo, hi = bounds[rank]
    index_path = "{0}.h5".format(save_file)
    # the index is written LAST; that it cannot be created ("w-", reference fitting.py:1632)
    # is said now (`_open_results`), not after the whole catalogue has been fitted
    taken = per_rank and rank == 0 and not resume and os.path.exists(index_path)
    return _Plan(rank, tuple(bounds), save_file, lo, hi, per_rank,
                 owner=not taken and (hi > lo if per_rank else rank == 0),
                 my_path=_part_path(save_file, rank) if per_rank else index_path,
                 my_rows=(hi - lo) if per_rank else bounds[-1][1],
                 my_first=lo if per_rank else 0, index_path=index_path, index_taken=taken)


class _SideGroup(object):
    """The gloo side group of the hand-off (`dist.new_group(backend="gloo")`: host memory to host
    memory, nothing is pickled and nothing passes through RCCL).  With one rank there is no group:
    a gather returns the caller's own vector and nothing else is ever called."""

    def __init__(self, world):
        import torch
        import torch.distributed as dist
        self.torch, self.dist, self.world = torch, dist, world
        self.group = dist.new_group(backend="gloo") if world > 1 else None

    def all_gather_i64(self, vec):
        """Every rank's `vec` (a few integers), as a `(world, len(vec))` array."""
        if self.group is None:
            return np.asarray(vec, dtype=np.int64)[None, :]
        torch = self.torch
        parts = [torch.empty(len(vec), dtype=torch.int64) for _ in range(self.world)]
        self.dist.all_gather(parts, torch.tensor(vec, dtype=torch.int64), group=self.group)
        return torch.stack(parts).numpy()

    def send(self, payload, dst):
        self.dist.send(self.torch.from_numpy(payload), dst=dst, group=self.group)

    def recv(self, nbytes, src):
        buf = self.torch.empty(nbytes, dtype=self.torch.uint8)
        self.dist.recv(buf, src=src, group=self.group)
        return buf.numpy()

    def broadcast_u8(self, state, src=0):
        """`state` (a uint8 array) of `src` into everybody's, in place."""
        if self.group is not None:
            self.dist.broadcast(self.torch.from_numpy(state), src=src, group=self.group)

    def destroy(self):
        if self.group is not None:
            self.dist.destroy_process_group(self.group)


def _open_results(plan, opts, data_labels):
    """`(out, open_error)`: this rank's `ResultsFile` (None unless it owns one), or why not."""
    from . import h5io
    if plan.index_taken:
        return None, OSError("fit_sharded: %s exists already" % plan.index_path)
    if not plan.owner:
        return None, None
    try:
        if opts.resume:
            # the interrupted file(s): rows whose `model_idx[:, 0]` still holds the sentinel
            # -99 were never fitted (reference fitting.py:1635)
            return h5io.ResultsFile.resume(plan.my_path, plan.my_rows, opts.Ndraws,
                                           opts.save_dar_draws), None
        lab = data_labels
        if plan.per_rank and lab is not None:
            lab = np.asarray(lab)[plan.lo:plan.hi]
        return h5io.ResultsFile(plan.my_path, plan.my_rows, opts.Ndraws, lab, opts.save_dar_draws,
                                running_io=opts.running_io), None
    except BaseException as e:
        return None, e


def _open_handshake(side, plan, out, open_error, resume):
    """One handshake for every way of opening: a rank that could not create / re-open its file
    says so before anybody enters the hand-off protocol, and EVERY rank raises (without it
    the others would wait for the failed rank in the first round of headers)."""
    oks = side.all_gather_i64([0 if open_error is not None else 1])
    bad = [r for r in range(side.world) if not int(oks[r, 0])]
    if not bad:
        return
    if out is not None:
        try:
            out.close()
            if not resume:
                os.remove(plan.my_path)     # created a moment ago, holds nothing: a rerun must not trip over it
        except BaseException:
            pass
    side.destroy()
    raise open_error or RuntimeError(
        "fit_sharded: rank(s) %s could not open their results file; this rank stops too"
        % ", ".join(str(r) for r in bad))


def _todo_mask(side, plan, out, Ndata):
    """The catalogue rows a resumed fit still has to do: what each owner reads from its file,
    and with one writer what rank 0 read, for everybody."""
    state = np.zeros(Ndata, dtype=np.uint8)
    if out is not None:
        state[plan.my_first + np.asarray(out.todo, dtype=np.int64)] = 1
    if not plan.per_rank:
        side.broadcast_u8(state)
    return state.astype(bool)


def _resume_runs(todo_mask, lo, hi):
    """The contiguous runs `[(a, b), ...]` of rows in `[lo, hi)` that this rank fits: all of them
    (`todo_mask` None), or those the boolean mask over the catalogue marks.  Each run is one `_fit`
    call seeded `seed0 + a` -- object i draws from stream `seed0 + i` as in the interrupted run,
    so the completed file equals an uninterrupted one."""
    if todo_mask is None:
        return [(lo, hi)] if hi > lo else []
    mine = np.flatnonzero(todo_mask[lo:hi]) + lo
    cuts = np.flatnonzero(np.diff(mine) != 1) + 1
    return [(int(r[0]), int(r[-1]) + 1) for r in np.split(mine, cuts) if r.size]


def _fitted_rows(bf, runs, data, data_err, data_mask, per_object, lnprior_ext, seed0, fit_kw):
    """(catalogue row, 13-tuple) of every row of `runs`, in row order.  `per_object`: keyword
    arrays (or None) with a row per object, sliced like the data, as `lnprior_ext`'s are;
    `fit_kw`: what is the same for every run.  Closing this generator closes the `_fit`
    generator in flight, which shuts its scan-ahead helper thread down."""
    for a, b in runs:
        rkw = dict(fit_kw)
        rkw.update((k, None if v is None else v[a:b]) for k, v in per_object.items())
        if lnprior_ext is not None:
            # per-object constraints: `_fit` sees objects a..b as 0..b-a
            rkw["lnprior_ext"] = {k: np.asarray(v)[a:b] for k, v in lnprior_ext.items()}
        g = bf._fit(data[a:b], data_err[a:b], data_mask[a:b], seed0=seed0 + a, **rkw)
        try:
            for k, res in enumerate(g):
                yield a + k, res
        finally:
            if hasattr(g, "close"):
                g.close()


def _pack_blocks(rows, chunk, rowdt, positions):
    """`(start, n, block)`: the `(row, 13-tuple)` pairs of `rows` packed `chunk` at a time into
    structured arrays of the file's own dtypes (`h5io.ResultsFile.row_dtype`); the first `n`
    entries of `block` are rows `start .. start + n`.  Every block is a fresh array (blocks sit
    in the queue while the next is filled) and holds consecutive rows only."""
    rows = iter(rows)
    exhausted = False
    pending = None                               # a row of the next run, already fitted
    while not exhausted:
        block = np.zeros(chunk, dtype=rowdt)
        n, start = 0, None
        with np.errstate(over="ignore"):
            while n < chunk:
                if pending is not None:
                    row, res = pending
                    pending = None
                else:
                    try:
                        row, res = next(rows)
                    except StopIteration:
                        exhausted = True
                        break
                if start is None:
                    start = row
                elif row != start + n:           # a new run: blocks hold consecutive rows
                    pending = (row, res)
                    break
                for name, pos in positions:
                    block[name][n] = res[pos]
                n += 1
        if n:
            yield start, n, block


class _HandOff(object):
    """The hand-off thread of one rank and its protocol.

    * The fit (`BruteForce._fit`, the caller's thread) packs every `chunk` finished objects into
      one block -- a structured array with the file's own dtypes (`h5io.ResultsFile.row_dtype`,
      18 KB per object at the defaults) -- and `put`s it into a bounded queue (`queue_depth`
      blocks: the only back-pressure is a writer slower than the fits).
    * This thread drains that queue over the side group: a round is one tiny `all_gather` of
      headers `(rows, first row, done, failed)` followed by point-to-point sends of exactly the
      rows that are ready -- a rank with nothing ready sends nothing and holds nobody up, so
      rank 0's shard, its unpacking and the writer's thread sit in no other rank's critical path.
    * Rank 0's thread gives the blocks to the asynchronous `ResultsFile` writer at their
      catalogue positions -- row `lo_r + ...`, the mapping of reference fitting.py:1734-1748.
      No rank holds more than `queue_depth * chunk` finished rows, rank 0 no more than a round
      of `world * chunk` on top, whatever the catalogue size.

    A failure anywhere -- a fit (`fail`), the writer (its errors are sticky), a hand-off -- is
    announced in the next round's headers; every rank's thread then ends with `error()` set and
    the next `put` or `check` raises it: none is left waiting in a collective.  That includes
    the writer's LAST blocks: when every rank has reported "done", the owners flush and close
    their files inside the protocol and a closing round of headers carries the outcome
    (`_close`).  With `writer="per_rank"` the queue carries nothing but "done": the fitting
    thread writes its own blocks and only the headers cross the side group.
    """

    def __init__(self, side, plan, out, rowdt, positions, queue_depth, write_index):
        self.side, self.plan, self.out = side, plan, out
        self.rowdt, self.positions, self.write_index = rowdt, positions, write_index
        self.q = queue.Queue(maxsize=max(1, int(queue_depth)))
        self.abort = threading.Event()
        self.local = self.remote = None          # this rank's own failure; the others', as told
        self.done = False
        self.thread = threading.Thread(target=self._run, name="brutus-shard-handoff", daemon=True)

    def error(self):
        """What stopped the protocol, this rank's own failure first; None while all is well.
        (`remote` is only ever set while `local` is None, and `local` after `remote` only by
        `fail`, i.e. when the fitting thread has an error of its own to raise.)"""
        return self.local or self.remote

    def check(self):
        if self.abort.is_set():                  # somebody failed: stop fitting
            raise self.error() or RuntimeError("fit_sharded aborted")

    def put(self, item):
        while True:
            self.check()
            try:
                self.q.put(item, timeout=0.05)
                return
            except queue.Full:
                continue

    def fail(self, e):
        """The fit raised `e`: tell the others, whatever the queue holds."""
        if not self.abort.is_set():
            self.local = self.local or e

    def _run(self):
        try:
            while self._round():
                pass
        except BaseException as e:               # the collective itself failed
            self.local = self.local or e
        finally:
            if self.error() is not None:
                self.abort.set()

    def _round(self):
        """Header round, then the rows that are ready; False when the protocol has ended."""
        # The failure state is read ONCE per round, before the queue: a block taken
        # from the queue is handed over in this round even if the fit raises while it
        # is on its way (the fitting thread runs on as soon as the queue has room), and
        # the failure goes into the next round's header.  Read after the `get`, the flag
        # could drop rows that were fitted before anything went wrong.
        failed = self.local is not None
        n, start, block, failed = self._take(failed)
        hdrs = self.side.all_gather_i64(self._header(n, start, failed))
        bad = np.flatnonzero(hdrs[:, 3])
        if bad.size:
            if self.local is None:
                self.remote = RuntimeError("fit_sharded: rank(s) %s failed; this rank stops too"
                                           % ", ".join(str(int(b)) for b in bad))
            return False
        try:
            self._deliver(hdrs, n, block)
        except BaseException as e:               # announced in the next round's headers: it
            self.local = e                       # does not end the thread
            return True
        if np.all(hdrs[:, 2] == 1) and not np.any(hdrs[:, 0]):
            self._close()
            return False
        return True

    def _take(self, failed):
        """`(n, start, block, failed)` of the next queue item, if there is one within 20 ms."""
        item = None
        if not self.done and not failed:
            try:
                item = self.q.get(timeout=0.02)
            except queue.Empty:
                pass
        n, start, block = 0, 0, None
        if item is not None:
            if item[0] == "rows":
                _, start, n, block = item
            elif item[0] == "done":
                self.done = True
            else:
                self.local = self.local or RuntimeError(item[1])
                failed = True
        return n, start, block, failed

    def _header(self, n, start, failed):
        return [n, start, 1 if self.done else 0, 1 if failed else 0]

    def _deliver(self, hdrs, n, block):
        if self.plan.rank == 0:
            got = []
            for r in range(self.side.world):     # every payload is received before any is
                nr = int(hdrs[r, 0])             # written: a failing write strands no sender
                if nr == 0:
                    continue
                if r == 0:
                    rows = block[:nr]
                else:
                    rows = self.side.recv(nr * self.rowdt.itemsize, src=r).view(self.rowdt)
                got.append((int(hdrs[r, 1]), rows))
            for first, rows in got:
                self.out.write_block(first, {name: rows[name] for name, _ in self.positions})
        elif n:
            self.side.send(block[:n].view(np.uint8).reshape(-1), dst=0)

    def _close(self):
        """Everything has been handed over -- but the writer is asynchronous: a failure in its
        last blocks (a full disk) only shows when the file is flushed and closed.  The owner does
        that HERE, and one more round of headers tells everybody how it went; otherwise it alone
        would raise after the threads have ended and the others would wait in the closing
        barrier."""
        if self.out is not None:
            try:
                self.out.close()
            except BaseException as e:
                self.local = e
        all_closed = self._closing_round()
        if self.plan.per_rank and all_closed:
            # every part is complete and closed: the index that presents them as the
            # reference's one file, and a second closing round for ITS verdict
            if self.plan.rank == 0:
                try:
                    self.write_index()
                except BaseException as e:
                    self.local = e
            self._closing_round()

    def _closing_round(self):
        """Everybody's verdict on the step just taken; True if all went well."""
        lasts = self.side.all_gather_i64([0, 0, 1, 0 if self.local is None else 1])
        badr = np.flatnonzero(lasts[:, 3])
        if badr.size and self.local is None:
            self.remote = RuntimeError(
                "fit_sharded: rank %s could not finish the results file; "
                "this rank stops too" % ", ".join(str(int(r)) for r in badr))
        return not badr.size


def fit_sharded(bf, data, data_err, data_mask, data_labels, save_file,
                seed0=0, rng="philox", chunk=256, rank0_share=1.0, queue_depth=4, writer="rank0",
                **fit_kwargs):
    """`BruteForce.fit` over all ranks of the default process group.

    Every rank fits the contiguous shard `shard_bounds(Ndata, world, rank0_share)[rank]` on
    its own GPU (no collective on the data path) and hands its finished rows to rank 0 in
    bounded pieces of `chunk` objects, WITHOUT the ranks ever waiting for each other's fits: a
    hand-off thread per rank drains a queue of `queue_depth` such blocks over a gloo side
    group, and rank 0's gives them to the asynchronous `ResultsFile` writer at their catalogue
    positions.  No rank holds more than `queue_depth * chunk` finished rows, rank 0 no more than
    `world * chunk` on top, whatever the catalogue size.  A failure anywhere -- a fit, the
    writer, a hand-off -- stops every rank: each raises, none is left waiting in a collective
    (`_HandOff` has the protocol).

    With `running_io=True` (default) the file on disk is current up to the last flush and
    `model_idx` is the last dataset of a block to be written, so a crash leaves the rows in
    flight unfitted (-99), never half-written.

    The bands that enter a fit are chosen once, from the whole catalogue's mask (a rank whose
    shard happens to lack a band must not run other kernel instantiations than its peers; up
    to three engines -- band sets -- stay resident per process).  Object `i` draws from its
    own stream keyed `seed0 + i`, so the file is
    identical for any number of ranks (the reference's single sequential
    stream, fitting.py:2039-2053, would make results depend on the sharding):
    `rng="philox"` (default) uses `rng.PhiloxRandomState(seed0 + i)`, which
    lets `lnpost` run on the GPU for the built-in priors; `rng="numpy"` uses
    `numpy.random.RandomState(seed0 + i)` (device `lnpost` as well; the host stage,
    optionally spread over `bf.host_workers` processes, for user prior hooks).

    `fit_kwargs` are `BruteForce.fit` keyword arguments (`lnprior_ext` arrays
    are sliced to each rank's rows).  `resume=True` completes an interrupted
    `running_io=True` file instead of creating one: rank 0 reads which rows still hold the
    sentinel, every rank fits the unfinished rows of its shard (same per-object streams, so
    the completed file equals an uninterrupted run's, for any number of ranks before and
    after).  Returns the number of objects this rank fitted; `fit_sharded.last_stats` holds this rank's
    timings (`fit_s`: until its last row was packed, `total_s`).

    `writer="per_rank"` takes the funnel out altogether: every rank writes the rows of ITS shard
    to `{save_file}.rNN.h5` (same datasets, `hi - lo` rows, its own asynchronous libhdf5 writer;
    nothing but the tiny headers crosses the side group), and when all are closed rank 0 writes
    `{save_file}.h5` as an INDEX: the 13 datasets as HDF5 virtual datasets that map row range
    `[lo_r, hi_r)` onto part `r` (`h5io.write_virtual_index`; the part files must stay beside it,
    `h5io.materialize` copies everything into one plain file when that is wanted).  Readers --
    h5py, `h5io.read_dataset` -- see the reference's layout.  With one writer 8 ranks x 25 k
    objects/s x 18 KB = 3.6 GB/s would pass through one gloo receiver and one libhdf5 thread;
    per rank it is 0.45 GB/s into a file of its own.  `resume=True` re-opens every rank's part
    (same number of ranks as the interrupted run).
    """
    import torch.distributed as dist
    from . import h5io
    rank, world = dist.get_rank(), dist.get_world_size()
    opts, skw, fkw = _split_fit_kwargs(fit_kwargs)
    chunk = max(1, int(chunk))
    (data, data_err, data_mask, data_labels, data_coords, lnprior, lngalprior,
     lndustprior, av_gauss, wt_thresh, _) = bf._setup(
        data, data_err, data_mask, data_labels, **skw)
    Ndata = data.shape[0]
    t_start = time.time()
    plan = _make_plan(rank, shard_bounds(Ndata, world, rank0_share), writer, save_file, opts.resume)
    side = _SideGroup(world)                     # host-to-host hand-off
    out, open_error = _open_results(plan, opts, data_labels)
    _open_handshake(side, plan, out, open_error, opts.resume)
    runs = _resume_runs(_todo_mask(side, plan, out, Ndata) if opts.resume else None,
                        plan.lo, plan.hi)
    nmine = sum(b - a for a, b in runs)
    per_object = {k: None if skw.get(k) is None else np.asarray(skw[k])
                  for k in ("parallax", "parallax_err")}
    gen = _fitted_rows(
        bf, runs, data, data_err, data_mask, dict(per_object, data_coords=data_coords),
        opts.lnprior_ext, seed0,
        dict(fkw, lnprior=lnprior, lngalprior=lngalprior, lndustprior=lndustprior,
             av_gauss=av_gauss, wt_thresh=wt_thresh, Ndraws=opts.Ndraws,
             return_distreds=opts.save_dar_draws,
             rstate_per_object="philox" if rng == "philox" else None))
    rowdt, positions = h5io.ResultsFile.row_dtype(opts.Ndraws, opts.save_dar_draws)
    handoff = _HandOff(side, plan, out, rowdt, positions, queue_depth, functools.partial(
        h5io.write_virtual_index, plan.index_path, Ndata, opts.Ndraws, opts.save_dar_draws,
        data_labels, plan.index_parts(), overwrite=opts.resume))
    handoff.thread.start()
    fit_error = t_fit = close_error = None
    try:
        bf._catalogue_mask = data_mask       # one band set for all ranks and runs (BruteForce._bands_for)
        try:
            for start, n, block in _pack_blocks(gen, chunk, rowdt, positions):
                if plan.per_rank:            # written here, at `start - lo` of this rank's part
                    handoff.check()
                    out.write_block(start - plan.lo,
                                    {name: block[name][:n] for name, _ in positions})
                else:
                    handoff.put(("rows", start, n, block))
            t_fit = time.time() - t_start
            handoff.put(("done",))
        except BaseException as e:
            fit_error = e
            handoff.fail(e)
        handoff.thread.join()
    finally:
        bf._catalogue_mask = None
        gen.close()                          # and with it the `_fit` generator in flight
        if out is not None:
            try:
                out.close()
            except BaseException as e:       # (sticky writer error: reported below)
                close_error = e
        side.destroy()
    err = fit_error or handoff.error() or close_error
    if err is not None:
        raise err
    fit_sharded.last_stats = {"fit_s": t_fit, "total_s": time.time() - t_start,
                              "objects": nmine, "writer": writer}
    dist.barrier()
    return nmine
