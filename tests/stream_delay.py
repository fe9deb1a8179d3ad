"""A delayed producer for the stream-order tests (tests/test_gpu_stream_order.py): work that keeps a torch side stream busy for a known time, so that a library
entry which fails to wait for the caller's stream, or for another handle's, reads what was there BEFORE the producer ran — a wrong answer, never a fault.

The delay is torch.cuda._sleep(cycles), calibrated once per Delay with two events.  Two torch streams can share a hardware queue (a process has four here), and
work queued behind the delay on the same queue would wait for it whatever the library does.  So a Delay makes FOUR side streams, every check runs with the
delay on each of them in turn, and every Delay carries its own proof that the delay delays: control(s, s2) fills a buffer with A, queues the delay and a fill
with B on s, copies the buffer to the host on s2 at once — A must arrive — and B after s has drained.  A module's checks mean something only if the control
is stale (A arrived) on at least one ordered pair of side streams: Delay.require_effective() FAILS the module otherwise; it never skips.

How long.  measure() (python tests/stream_delay.py) finds the shortest delay of its ladder at which every pair of side streams that is stale at 50 ms is stale
in 20 of 20 tries; twice that, capped at MAX_DELAY_MS, is the least delay a check may use.  Measured on an MI355X with four hardware queues:
    shortest delay, stale 20 of 20:  0.05 ms (the ladder's first step; all 12 ordered pairs)        doubled: CONTROL_DELAY_MS = 0.1 ms
The control's reader touches the buffer within microseconds of the producer's launch.  A library entry does not: dge_regions_locate_device,
dge_flows_add_trips_device and the .seq writer create a stream and allocate their scratch before their first kernel reads anything, and a delay that has run
out by then shows nothing, whatever the entry fails to wait for (with 0.1 ms a library without those waits passes their checks; it is the control that passes
so early, not the entries).  So the checks use DELAY_MS = 5 ms — fifty times the control's figure, far beyond any entry's preamble, and still 4 streams x
some 40 delays, under a second for the whole file.  A longer delay can only show more: what goes unordered for 0.1 ms goes unordered for 5.

Rules the checks keep (this module cannot enforce them): every tensor is allocated beforehand on the default stream and lives until the check's final
torch.cuda.synchronize(); the stale and the fresh contents of every buffer are both valid arguments of the entry under test."""
import contextlib

N_SIDE = 4
MAX_DELAY_MS = 200.0
CONTROL_DELAY_MS = 0.1    # what measure() gave, doubled
DELAY_MS = 5.0            # what the checks use (the docstring says why)
assert CONTROL_DELAY_MS <= DELAY_MS <= MAX_DELAY_MS
A, B = 0x5A, 0x3C         # the control's two byte values


class Delay:
    def __init__(self, device="cuda:0", delay_ms=None):
        import torch
        self.torch = torch
        self.device = torch.device(device)
        self.delay_ms = min(float(DELAY_MS if delay_ms is None else delay_ms), MAX_DELAY_MS)
        self.side = [torch.cuda.Stream(self.device) for _ in range(N_SIDE)]
        self._buf = torch.empty(1 << 16, dtype=torch.uint8, device=self.device)
        self._pin = torch.empty(1 << 16, dtype=torch.uint8).pin_memory()
        self.cycles_per_ms = self._calibrate()
        self.stale_pairs = None

    def _calibrate(self):
        """_sleep's cycles per millisecond: 4 M cycles between two events, after a warm-up (the first launch loads the kernel)."""
        torch = self.torch
        s = self.side[0]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            torch.cuda._sleep(100_000)
            s.synchronize()
            e0.record(s); torch.cuda._sleep(4_000_000); e1.record(s)
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0.05, "torch.cuda._sleep(4e6) took %.4f ms: it does not sleep" % ms
        return 4_000_000 / ms

    def sleep(self, ms=None):
        """queues the delay on the CURRENT torch stream"""
        self.torch.cuda._sleep(int(self.cycles_per_ms * (self.delay_ms if ms is None else ms)))

    @contextlib.contextmanager
    def delayed(self, s, ms=None):
        """with D.delayed(s): <torch ops> — the ops are queued on s behind the delay; everything queued before is finished first (the delay starts at once)"""
        self.torch.cuda.synchronize(self.device)
        with self.torch.cuda.stream(s):
            self.sleep(ms)
            yield s

    def read_on(self, s2, t):
        """the bytes of tensor t as they stand for stream s2 NOW: an asynchronous copy into pinned memory queued on s2, then a wait for s2 alone -> numpy"""
        torch = self.torch
        pin = torch.empty(t.shape, dtype=t.dtype).pin_memory()
        with torch.cuda.stream(s2):
            pin.copy_(t, non_blocking=True)
        s2.synchronize()
        return pin.numpy().copy()

    def other(self, s):
        """a side stream that is not s: the one after it"""
        return self.side[(self.side.index(s) + 1) % N_SIDE]

    def control(self, s, s2, ms=None):
        """-> True when the reader on s2 saw the STALE buffer, i.e. the delay on s held the producer back and s2 did not queue up behind it.  Asserts that the
        buffer is one of the two fills as a whole, and that the fresh fill is there once s has drained."""
        torch = self.torch
        self._buf.fill_(A)
        with self.delayed(s, ms):
            self._buf.fill_(B)
        with torch.cuda.stream(s2):
            self._pin.copy_(self._buf, non_blocking=True)
        s2.synchronize()
        early = self._pin.numpy().copy()
        s.synchronize()
        with torch.cuda.stream(s2):
            self._pin.copy_(self._buf, non_blocking=True)
        s2.synchronize()
        late = self._pin.numpy().copy()
        torch.cuda.synchronize(self.device)
        assert (late == B).all(), "the control's producer did not run"
        assert (early == A).all() or (early == B).all(), "the control's buffer is torn"
        return bool((early == A).all())

    def require_effective(self):
        """The control on every ordered pair of side streams -> the stale pairs [(producer, reader)].  None stale: the module fails — its checks would pass on a
        library that waits for nothing."""
        if self.stale_pairs is None:
            self.stale_pairs = [(i, j) for i in range(N_SIDE) for j in range(N_SIDE) if i != j and self.control(self.side[i], self.side[j])]
        assert self.stale_pairs, ("the delay was not effective: with %.2f ms on a side stream, no reader on another side stream saw the stale buffer "
                                  "(%d side streams, every ordered pair tried)" % (self.delay_ms, N_SIDE))
        return self.stale_pairs


LADDER_MS = (0.05, 0.1, 0.2, 0.5, 1.0, 2.0, 5.0, 10.0, 20.0, 50.0, 100.0)


def measure(tries=20, out=print):
    """-> (shortest delay of LADDER_MS at which every pair stale at 50 ms is stale in `tries` of `tries`, or None; that delay doubled and capped)"""
    D = Delay(delay_ms=50.0)
    out("_sleep: %.0f cycles per ms" % D.cycles_per_ms)
    pairs = D.require_effective()
    out("stale at 50 ms: %d of %d ordered pairs: %s" % (len(pairs), N_SIDE * (N_SIDE - 1), pairs))
    shortest = None
    for ms in LADDER_MS:
        hits = {p: sum(D.control(D.side[p[0]], D.side[p[1]], ms) for _ in range(tries)) for p in pairs}
        out("%7.2f ms: stale %s of %d" % (ms, sorted(set(hits.values())), tries))
        if shortest is None and all(h == tries for h in hits.values()):
            shortest = ms
    delay = None if shortest is None else min(2 * shortest, MAX_DELAY_MS)
    out("shortest %s ms -> DELAY_MS %s" % (shortest, delay))
    return shortest, delay


if __name__ == "__main__":
    measure()
