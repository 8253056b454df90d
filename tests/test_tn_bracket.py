"""The grouped weight-gradient bracket as a protocol, at the C ABI (include/rgbnm.h: rgbnm_gemm_tn_group_begin / _begin_n /
_begin_id / _abort / _end; gemm.hip: the thread_local queue behind them).

tests/test_kernel_edges.py::test_gemm_tn_group_bracket_flushes covers the flush causes of one flat bracket; this file covers
what a caller can get wrong around it: nesting (a _begin inside an open bracket JOINS it), naming, _abort from the owning
thread and from another one, an element-type change and non-groupable jobs inside a bracket, and an _end without a _begin.
If any of these goes wrong a weight gradient is silently never written, so every scenario checks both directions:
"ran" is tests/test_kernel_edges.py's tn_check (guards, every element against fp64), "dropped" is dW and db still holding
the canary bit for bit while no gemm_tn* kernel was dispatched.

Every scenario runs on a fresh host thread (Owner): the bracket state is thread_local, so a scenario that fails half way cannot
leave a bracket open for the tests that follow.  Only real, live, guarded buffers are handed to the library, and they stay
alive until after the scenario's last synchronize: a job that is launched although it should have been dropped writes memory
the test owns and is caught by the canaries.  Jobs: bf16, M = 64, No = Ki = 192 (two 128 x 192 tiles), tn_pipe = 1.

Run time on one MI355X: 9 tests, 2 s after the first profiler start-up (4 s as a file of its own).
"""
import queue
import threading

import pytest
import torch

from kernel_check import Worst, guarded, launched
from rgb_no_more_amd import lib as L
from test_hip_kernels import option  # noqa: F401  (fixture: set a runtime switch for one test)
from test_fp16_tuned_kernels import is_f16
from test_kernel_edges import tn_check, tn_operands, tn_outputs

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
M0, NO0, KI0 = 64, 192, 192


class Owner:
    """A fresh host thread that runs what the test hands it, one call at a time: the thread whose thread_local queue the
    scenario is about.  The test's own thread keeps the profiler (kernel_check.launched) and the checks."""

    def __init__(self):
        self.todo, self.done = queue.Queue(), queue.Queue()
        self.thread = threading.Thread(target=self._loop)

    def _loop(self):
        torch.cuda.set_device(0)
        while True:
            fn = self.todo.get()
            if fn is None:
                return
            try:
                self.done.put((fn(), None))
            except BaseException as e:  # noqa: BLE001  (handed to the test's thread)
                self.done.put((None, e))

    def __call__(self, fn):
        self.todo.put(fn)
        res, err = self.done.get()
        if err is not None:
            raise err
        return res

    def __enter__(self):
        self.thread.start()
        return self

    def __exit__(self, *exc):
        self.todo.put(None)
        self.thread.join()


class Job:
    """One rgbnm_gemm_tn call: NaN-padded operands, guarded dW / db / workspace."""

    def __init__(self, seed, dt=BF16, M=M0, No=NO0, Ki=KI0, name=""):
        self.dt, self.M, self.No, self.Ki, self.name = dt, M, No, Ki, name or f"job{seed}"
        self.dY, self.X, self.ldy, self.ldx = tn_operands(dt, M, No, Ki, 1000 + 10 * seed, pad=bool(seed % 2))
        self.dW, self.db = tn_outputs(No, Ki, 0, True, seed)
        self.wsb = L.lib().rgbnm_gemm_tn_workspace(M, No, Ki)
        self.ws = guarded(self.wsb // 4, None, F32)

    def submit(self):
        L.check(L.lib().rgbnm_gemm_tn(L.dt_of(self.dt), self.dY.data_ptr(), self.ldy, self.X.data_ptr(), self.ldx,
                                      self.dW.t.data_ptr(), self.db.t.data_ptr(), self.M, self.No, self.Ki, 0, 0,
                                      self.ws.t.data_ptr(), self.wsb, L.stream()), self.name)

    def untouched(self, where):
        """dW, db, their margins and the workspace hold the canary bit for bit: the job never ran."""
        for what, g in (("dW", self.dW), ("db", self.db), ("workspace", self.ws)):
            n = int((g.raw != g.canary).sum())
            assert n == 0, f"{where}: {self.name} {what}: {n} elements written although the job must not have run"

    def ran(self, where, worst):
        self.ws.check(f"{where}: {self.name} workspace", written=False)
        tn_check(self.dY, self.X, self.dW, self.db, 0, 0, None, f"{where}: {self.name}", worst, "bracket")


def tn_launches(names):
    return [n for n in names if "gemm_tn" in n]


def step(own, fn, want, where):
    """Run fn on the owner thread, assert that it dispatched exactly `want` weight-gradient kernels."""
    _, names = launched(lambda: own(fn))
    got = tn_launches(names)
    assert len(got) == want, f"{where}: {len(got)} weight-gradient launches, expected {want}: {sorted(set(names))}"
    return names


def end():
    L.check(L.lib().rgbnm_gemm_tn_group_end(L.stream()), "group_end")


def test_inner_begin_joins_the_open_bracket(option):
    """A _begin_n inside an open bracket joins: nothing runs at the inner _end, everything in ONE launch at the outer."""
    option("tn_pipe", 1)
    lib = L.lib()
    worst = Worst()
    a, b, c = Job(1), Job(2), Job(3)

    def inner():
        lib.rgbnm_gemm_tn_group_begin_n(8)
        a.submit()
        lib.rgbnm_gemm_tn_group_begin_n(8)
        b.submit()
        end()

    def outer():
        c.submit()
        end()
    with Owner() as own:
        step(own, inner, 0, "inner _end")
        for j in (a, b):
            j.untouched("after the inner _end")
        step(own, outer, 1, "outer _end")
        for j in (a, b, c):
            j.ran("after the outer _end", worst)
        step(own, end, 0, "_end after the bracket closed")


def test_begin_id_names_only_an_outermost_bracket(option):
    """_begin_id inside an open bracket joins it without renaming it: _abort of the inner id changes nothing, _abort of the
    outer id drops the queue.  Inside an UNNAMED bracket an inner _begin_id gives no name either."""
    option("tn_pipe", 1)
    lib = L.lib()
    worst = Worst()
    a, b, c, d, e = (Job(i) for i in range(11, 16))

    def named():
        lib.rgbnm_gemm_tn_group_begin_id(8, 7001)
        a.submit()
        lib.rgbnm_gemm_tn_group_begin_id(8, 7002)      # joins: the bracket keeps the name 7001
        b.submit()
        lib.rgbnm_gemm_tn_group_abort(7002)            # names no open bracket: parked, never matched
        c.submit()                                     # touches the queue: nothing to drop
        end()                                          # the inner _end

    def unnamed():
        lib.rgbnm_gemm_tn_group_begin_n(8)
        lib.rgbnm_gemm_tn_group_begin_id(8, 7003)      # joins an unnamed bracket: still unnamed
        e.submit()
        lib.rgbnm_gemm_tn_group_abort(7003)            # names no open bracket: nothing dropped
        end()
        end()
    with Owner() as own:
        step(own, named, 0, "named bracket, inner id aborted")
        for j in (a, b, c):
            j.untouched("inner id aborted")
        step(own, lambda: lib.rgbnm_gemm_tn_group_abort(7001), 0, "abort of the outer id")
        step(own, d.submit, 1, "job after the abort")  # the bracket is closed: launches at once, alone
        d.ran("after the abort", worst)
        for j in (a, b, c):
            j.untouched("outer id aborted")
        step(own, unnamed, 1, "unnamed outer bracket")
        e.ran("inner name inside an unnamed bracket", worst)


def test_abort_on_the_own_thread_drops_at_once(option):
    option("tn_pipe", 1)
    lib = L.lib()
    worst = Worst()
    a, b, c = Job(21), Job(22), Job(23)

    def dropped():
        lib.rgbnm_gemm_tn_group_begin_id(8, 8001)
        a.submit()
        b.submit()
        lib.rgbnm_gemm_tn_group_abort(8001)
    with Owner() as own:
        step(own, dropped, 0, "own-thread abort")
        step(own, c.submit, 1, "job after the abort")  # no bracket is open any more: ungrouped, at once
        c.ran("after own-thread abort", worst)
        step(own, end, 0, "_end after the abort")
        for j in (a, b):
            j.untouched("own-thread abort")


def test_abort_from_another_thread_takes_effect_at_the_owners_next_touch(option):
    option("tn_pipe", 1)
    lib = L.lib()
    worst = Worst()
    a, b, c, d = Job(31), Job(32), Job(33), Job(34)

    def first():
        lib.rgbnm_gemm_tn_group_begin_id(8, 9001)
        a.submit()
        b.submit()

    def again():                                       # the abort was consumed: the same name can be used again
        lib.rgbnm_gemm_tn_group_begin_id(8, 9001)
        d.submit()
        end()
    with Owner() as own:
        step(own, first, 0, "queued")
        lib.rgbnm_gemm_tn_group_abort(9001)            # THIS thread is not the owner
        for j in (a, b):
            j.untouched("aborted from another thread")
        step(own, c.submit, 1, "owner's next job")     # sees the abort: drops a and b, closes the bracket, runs c alone
        c.ran("after the foreign abort", worst)
        step(own, end, 0, "_end of the aborted bracket")
        step(own, again, 1, "a new bracket of the same name")
        d.ran("new bracket", worst)
        for j in (a, b):
            j.untouched("foreign abort")


def test_abort_of_zero_or_an_unknown_id_changes_nothing(option):
    option("tn_pipe", 1)
    lib = L.lib()
    worst = Worst()
    a, b = Job(41), Job(42)

    def bracket():
        lib.rgbnm_gemm_tn_group_begin_id(8, 9101)
        a.submit()
        lib.rgbnm_gemm_tn_group_abort(0)
        lib.rgbnm_gemm_tn_group_abort(9102)
        b.submit()
    with Owner() as own:
        step(own, bracket, 0, "still queued")
        lib.rgbnm_gemm_tn_group_abort(0)               # and from another thread
        lib.rgbnm_gemm_tn_group_abort(9103)
        for j in (a, b):
            j.untouched("before _end")
        step(own, end, 1, "_end")
        for j in (a, b):
            j.ran("abort(0) / abort(unknown)", worst)


def test_element_type_change_flushes_what_is_queued(option):
    """fp16 (f16_tuned = 1) after bf16: the bf16 jobs run when the fp16 job arrives, the fp16 job at _end."""
    option("tn_pipe", 1)
    option("f16_tuned", 1)
    lib = L.lib()
    worst = Worst()
    a, b, h = Job(51), Job(52), Job(53, dt=F16)

    def queue_bf16():
        lib.rgbnm_gemm_tn_group_begin_n(8)
        a.submit()
        b.submit()
    with Owner() as own:
        step(own, queue_bf16, 0, "bf16 queued")
        step(own, h.submit, 1, "fp16 job arrives")
        for j in (a, b):
            j.ran("flushed by the type change", worst)
        h.untouched("fp16 job before _end")
        names = step(own, end, 1, "_end")
        assert all(is_f16(n) for n in tn_launches(names)), names
        h.ran("fp16 at _end", worst)


def test_non_groupable_jobs_run_at_once_and_leave_the_queue(option):
    """M % 64 != 0, Ki % 192 != 0 and fp32 jobs inside a bracket launch immediately; the queued job still waits for _end."""
    option("tn_pipe", 1)
    lib = L.lib()
    worst = Worst()
    a = Job(61)
    odd = [Job(62, M=65, name="M=65"), Job(63, Ki=128, name="Ki=128"), Job(64, dt=F32, name="fp32")]

    def first():
        lib.rgbnm_gemm_tn_group_begin_n(8)
        a.submit()
    with Owner() as own:
        step(own, first, 0, "queued")
        for j in odd:
            step(own, j.submit, 1, j.name)
            j.ran("inside the bracket", worst)
            a.untouched(f"after {j.name}")
        step(own, end, 1, "_end")
        a.ran("after _end", worst)


def test_end_without_begin_is_ok_and_launches_nothing(option):
    option("tn_pipe", 1)
    with Owner() as own:
        rc, names = launched(lambda: own(lambda: L.lib().rgbnm_gemm_tn_group_end(L.stream())))
    assert rc == 0 and names == [], (rc, names)


def test_unnamed_bracket_left_open_is_joined_and_a_named_one_recovers(option):
    """include/rgbnm.h: an unnamed bracket must be closed by the thread that opened it.  The library cannot tell a bracket
    whose pass died before its _end from one that is still open, so a later _begin_n on that thread JOINS the dead one: its
    _end only un-nests, and neither the dead pass's job nor the new one runs until one more _end closes the dead bracket
    (then both run: the operands here are alive).  A pass that can die takes a named bracket instead: _abort(id) drops the
    dead pass's jobs and the next bracket is a fresh one.

    History: the header used to promise that such a _begin "starts from an empty queue".  rgbnm_tn_defer_begin_n joined
    before it reached its reset, so the promise could not be kept: run as the header had it on one MI355X (begin_n, A, no
    _end, begin_n, B, _end), no weight-gradient kernel was launched and neither dW was written."""
    option("tn_pipe", 1)
    lib = L.lib()
    worst = Worst()
    a, b, c, d = Job(71), Job(72), Job(73), Job(74)

    def dead_then_new():
        lib.rgbnm_gemm_tn_group_begin_n(8)
        a.submit()                                     # ... the pass dies here: no _end
        lib.rgbnm_gemm_tn_group_begin_n(8)
        b.submit()
        end()
    with Owner() as own:
        step(own, dead_then_new, 0, "joined the dead bracket")
        for j in (a, b):
            j.untouched("dead unnamed bracket")
        step(own, end, 1, "the _end the dead pass owed")
        for j in (a, b):
            j.ran("dead bracket closed", worst)

    def named_dead_then_new():
        lib.rgbnm_gemm_tn_group_begin_id(8, 9201)
        c.submit()                                     # ... the pass dies here
        lib.rgbnm_gemm_tn_group_abort(9201)            # whoever notices it
        lib.rgbnm_gemm_tn_group_begin_id(8, 9202)
        d.submit()
        end()
    with Owner() as own:
        step(own, named_dead_then_new, 1, "named recovery")
        c.untouched("dead named bracket")
        d.ran("the bracket after the abort", worst)
        step(own, end, 0, "nothing left open")
