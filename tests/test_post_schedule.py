"""The hand-over schedule of the device `lnpost` stage (`fitting._post_schedule`) with stand-in
stages: no GPU, no torch.  Every stage appends (event, batch, thread) to one locked list; the
assertions read the order of that list.  Every wait in a stand-in has a timeout, so that a wrong
schedule fails instead of hanging."""
import threading
import time

import pytest

from brutus_amd.fitting import _PostStages, _post_schedule

WAIT = 5.0          # seconds a stand-in waits for another stage before it gives up
ROWS = 2            # rows per batch


class Fakes(object):
    """Stand-in stages over `nbatch` batches scanned by `nE` engines.  `decline`: batches whose
    phase 1 declines.  `late`: seconds phase 2 sleeps.  `gate`: phase 2 of batch j returns only
    once scan j + 3 has started.  `fail` = (stage name, batch): that stage raises `Boom`."""

    class Boom(Exception):
        pass

    def __init__(self, nbatch, nE, decline=(), late=0., gate=False, fail=None):
        self.nbatch, self.nE, self.decline = nbatch, nE, set(decline)
        self.late, self.gate, self.fail = late, gate, fail
        self.lock = threading.Lock()
        self.events = []
        self.flags = {}           # (event, batch) -> threading.Event
        self.running = 0
        self.timeouts = []
        self.in_slot = {}
        self.stages = _PostStages(self.scan, self.args, self.begin, self.end, self.whole,
                                  self.rows)

    # -- bookkeeping --------------------------------------------------------------------
    def flag(self, name, k):
        with self.lock:
            return self.flags.setdefault((name, k), threading.Event())

    def log(self, name, k):
        with self.lock:
            self.events.append((name, k, threading.current_thread()))
        self.flag(name, k).set()

    def wait_for(self, name, k, who):
        if not self.flag(name, k).wait(WAIT):
            with self.lock:
                self.timeouts.append((who, "waited for", name, k))

    def enter(self, name, k):
        with self.lock:
            self.running += 1
        self.log(name + "_start", k)
        if self.fail == (name, k):
            self.leave(name, k)
            raise self.Boom("%s %d" % (name, k))

    def leave(self, name, k):
        self.log(name + "_done", k)
        with self.lock:
            self.running -= 1

    def at(self, name, k):
        """Position of an event in the log (None: it never happened)."""
        for i, (n, kk, _) in enumerate(self.events):
            if (n, kk) == (name, k):
                return i
        return None

    def threads(self, name):
        return set(t for n, _, t in self.events if n == name)

    # -- the stages ---------------------------------------------------------------------
    def scan(self, k):
        self.enter("scan", k)
        self.leave("scan", k)
        return ("scanned", k)

    def args(self, k):
        self.log("args", k)
        return ("call", k)

    def begin(self, k, slot, scanned, call, after_jump):
        assert scanned == ("scanned", k) and call == ("call", k) and slot == k % 2
        with self.lock:
            self.running += 1
        self.log("begin_start", k)
        try:
            self.log("jump_in", k)
            after_jump()
            self.log("jump_out", k)
            # phase 2 of the previous batch was submitted in there -- if it went through
            # phase 1 -- and so starts now: the finisher is free, its last batch was waited for
            if self.at("begin_ok", k - 1) is not None:
                self.wait_for("end_start", k - 1, ("begin", k))
            if self.fail == ("begin", k):
                raise self.Boom("begin %d" % k)
            if k in self.decline:
                return False
            self.in_slot[slot] = k
            self.log("begin_ok", k)
            return True
        finally:
            self.leave("begin", k)

    def end(self, slot):
        k = self.in_slot[slot]
        self.enter("end", k)
        if self.late:
            time.sleep(self.late)
        if self.gate and k + 3 < self.nbatch:
            self.wait_for("scan_start", k + 3, ("end", k))
        self.leave("end", k)
        return ("result", k)

    def whole(self, k, scanned, call):
        assert scanned == ("scanned", k) and call == ("call", k)
        self.enter("whole", k)
        self.leave("whole", k)
        return ("result", k)

    def rows(self, k, scanned, result):
        assert scanned == ("scanned", k) and result == ("result", k)
        self.log("rows", k)
        return [(k, j) for j in range(ROWS)]

    # -- what every run has to satisfy --------------------------------------------------
    def check(self, pipelined, upto=None):
        """The order rules, over the batches that were started (`upto`: the run was cut short)."""
        assert not self.timeouts, self.timeouts
        assert self.running == 0
        me = threading.current_thread()
        for name in ("args", "begin_start", "whole_start", "rows"):
            assert self.threads(name) <= {me}, name
        helpers = self.threads("scan_start") | self.threads("end_start")
        assert all(not t.is_alive() for t in helpers if t is not me)     # both executors are down
        if pipelined:
            assert me not in helpers and not (self.threads("scan_start") & self.threads("end_start"))
        done = lambda k: self.at("end_done", k) if self.at("end_done", k) is not None \
            else self.at("whole_done", k)
        for k in range(self.nbatch):
            s, b = self.at("scan_start", k), self.at("begin_start", k)
            if s is not None and k >= self.nE:
                # engine k % nE is free: batch k - nE is finished, by phase 2 or by the whole call
                assert done(k - self.nE) is not None and done(k - self.nE) < s, ("engine", k)
            if b is not None and k >= 2 and self.at("begin_ok", k - 2) is not None:
                # slot k % 2 is free: phase 2 of batch k - 2 has returned
                assert self.at("end_done", k - 2) < b, ("slot", k)
            e = self.at("end_start", k)
            if e is not None and self.at("begin_start", k + 1) is not None:
                # phase 2 of k goes off inside the after_jump of phase 1 of k + 1, not earlier
                assert self.at("jump_in", k + 1) < e, ("after_jump", k)
            if not pipelined:
                assert b is None and e is None
            elif upto is None:
                assert (self.at("begin_ok", k) is None) == (k in self.decline)
                assert (self.at("whole_start", k) is not None) == (k in self.decline)
                assert (e is not None) == (k not in self.decline)


def declines(pattern, n):
    return {"none": (), "first": (0,), "middle": (n // 2,), "last": (n - 1,),
            "all": tuple(range(n))}[pattern]


def expected(n):
    return [(k, j) for k in range(n) for j in range(ROWS)]


@pytest.mark.parametrize("pattern", ["none", "first", "middle", "last", "all"])
@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("nbatch", range(1, 10))
def test_rows_in_order_and_every_hand_over(nbatch, pipelined, pattern):
    """1 .. 9 batches, two and four engines, every decline pattern: each batch comes out once,
    in order, and the slot / engine / after_jump rules hold."""
    f = Fakes(nbatch, 4 if pipelined else 2, decline=declines(pattern, nbatch))
    assert list(_post_schedule(nbatch, f.stages, True, pipelined)) == expected(nbatch)
    f.check(pipelined)


def test_without_a_scan_ahead_everything_runs_on_the_callers_thread():
    f = Fakes(3, 2)
    assert list(_post_schedule(3, f.stages, False, False)) == expected(3)
    f.check(False)
    assert f.threads("scan_start") == {threading.current_thread()}


@pytest.mark.parametrize("nbatch", [4, 5, 9])
def test_scan_is_submitted_before_the_wait_for_the_slot(nbatch):
    """Phase 2 of batch k - 2 returns only once scan k + 1 has started: the schedule submits that
    scan BEFORE it waits for the slot (submitted behind the wait it would land on the next
    batch's jump-ahead kernels), so the run completes -- and needs the fourth engine for it."""
    f = Fakes(nbatch, 4, gate=True)
    assert list(_post_schedule(nbatch, f.stages, True, True)) == expected(nbatch)
    f.check(True)
    for k in range(nbatch - 3):
        assert f.at("scan_start", k + 3) < f.at("end_done", k)


@pytest.mark.parametrize("pattern", ["none", "middle"])
def test_a_late_phase_two_changes_nothing(pattern):
    f = Fakes(6, 4, decline=declines(pattern, 6), late=0.02)
    assert list(_post_schedule(6, f.stages, True, True)) == expected(6)
    f.check(True)


@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("stop", [1, 2 * ROWS, 3 * ROWS + 1])
def test_abandoning_the_generator_leaves_nothing_running(stop, pipelined):
    """close() after one row, at a batch boundary, inside a later batch: when it returns no
    stage runs and the helper threads are gone; a full run afterwards is complete."""
    f = Fakes(7, 4 if pipelined else 2, late=0.005)
    g = _post_schedule(7, f.stages, True, pipelined)
    got = [next(g) for _ in range(stop)]
    g.close()
    assert got == expected(7)[:stop]
    n = len(f.events)
    f.check(pipelined, upto=stop)
    time.sleep(0.02)
    assert len(f.events) == n          # nothing went on behind the caller's back
    f2 = Fakes(7, 4 if pipelined else 2)
    assert list(_post_schedule(7, f2.stages, True, pipelined)) == expected(7)
    f2.check(pipelined)


@pytest.mark.parametrize("fail", [("scan", 0), ("scan", 3), ("end", 0), ("end", 2), ("end", 4),
                                  ("whole", 1)])
def test_an_exception_in_a_helper_thread_reaches_the_caller(fail):
    decline = (1,) if fail[0] == "whole" else ()
    f = Fakes(5, 4, decline=decline, fail=fail)
    got = []
    with pytest.raises(Fakes.Boom, match="%s %d" % fail):
        for row in _post_schedule(5, f.stages, True, True):
            got.append(row)
    assert got == expected(5)[:len(got)] and len(got) <= fail[1] * ROWS
    f.check(True, upto=len(got))


@pytest.mark.parametrize("decline", [(), (2,)])
def test_phase_two_is_submitted_even_when_phase_one_raises_or_declines(decline):
    """after_jump fires whatever phase 1 does: phase 2 of batch 1 runs although phase 1 of
    batch 2 raised (or declined), and the executors are shut down after it."""
    f = Fakes(4, 4, decline=decline, fail=None if decline else ("begin", 2))
    g = _post_schedule(4, f.stages, True, True)
    if decline:
        assert list(g) == expected(4)
    else:
        with pytest.raises(Fakes.Boom, match="begin 2"):
            list(g)
    f.check(True, upto=0)
    assert f.at("jump_in", 2) < f.at("end_start", 1) and f.at("end_done", 1) is not None
