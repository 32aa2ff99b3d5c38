"""Packed or float?  The choice of BFS's level read-back, as bookkeeping alone: no GPU, no library call, no driver state.

The packed read-back's second half runs on HOST threads: on a busy machine it loses to the plain float copy ("The
read-back measures itself": 0.39 - 0.52 ms for the same call from one machine to the next, 0.39 - 0.55 within one process).  So the
driver (app.BFS._pull_push_bits) MEASURES: both ways are timed (whole call), the faster one by the MEDIAN of its last seven calls
is used, and every 32nd call tries the other one again.  The books are kept per schedule (pull and pull_push each have their own:
one exponential average for both was poisoned by the first calls of the second mode, which enqueue and record its graph -- 12 ms
-- and the mode measured second ran on the slower way, 33 % apart between two legs of one bench process).  The durations are
handed in, so the policy can be driven with synthetic times (tests/test_readback_arbiter.py).
"""
import collections
import statistics

# one book per schedule and slice read back: the driver keeps a defaultdict(ReadbackBook) by BookKey
BookKey = collections.namedtuple("BookKey", "N threshold back pull_only lo own")

WARM_CALLS = 2      # the first calls of a way enqueue / record its schedule: not what the steady state costs
WINDOW = 7          # the median is taken over a way's last WINDOW recorded calls
FLOAT_FROM = 8      # float is first tried on this call (the ones before warm up and record the packed way's graph)
RETRY_EVERY = 32    # calls % RETRY_EVERY == RETRY_EVERY - 1: the slower way is measured again


class ReadbackBook:
    """The measurements of one schedule: `packed` / `float` = median seconds of the way's last WINDOW recorded calls (None: not
    measured yet), `calls` = recorded calls of either way."""

    def __init__(self):
        self.packed = self.float = None
        self.calls = 0
        self._seen = {"packed": 0, "float": 0}
        self._times = {"packed": [], "float": []}

    def choose(self, can_pack, timed, pin):
        """-> as_bytes.  `pin` = GRAPHLILY_BFS_U8 ("2": always packed; "0" arrives as can_pack False).  A run that cannot pack,
        or whose schedule is being timed alone, takes can_pack and is not a measurement (the caller does not record it)."""
        if not can_pack or timed:
            return can_pack
        if pin == "2" or self.packed is None:
            return True
        if self.float is None:
            return self.calls < FLOAT_FROM
        better = self.packed <= self.float
        return better if self.calls % RETRY_EVERY != RETRY_EVERY - 1 else not better

    def record(self, way, seconds):
        """One whole call (`way`: "packed" or "float") took `seconds`."""
        seen = self._seen[way]
        self._seen[way] = seen + 1
        if seen >= WARM_CALLS:
            ts = self._times[way]
            ts.append(seconds)
            del ts[:-WINDOW]
            setattr(self, way, float(statistics.median(ts)))
        self.calls += 1

    def report(self, way):
        """What BFS.readback_ says after a recorded call that went `way`."""
        return {"way": way, "packed_ms": None if self.packed is None else round(self.packed * 1e3, 4),
                "float_ms": None if self.float is None else round(self.float * 1e3, 4)}

