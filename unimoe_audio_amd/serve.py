"""Continuous batching policy of a decode engine on per-row clocks: plain host code, no device, no library.

A queue of requests is served by a fixed number of rows.  Requests are admitted first in, first out, one per free row, at every
poll; between two polls the engine takes `poll_every` decode steps (as DecodeEngine.run() does between two reads of its flag); a row
whose request ended is retired at the poll that sees it, its result handed out, and the row is free for the next request.

The engine is anything with

    admit(row, request)       put `request` into the free row `row`
    steps(n)                  take n decode steps
    poll() -> state           one read of the engine's state
    row_done(state, row)      whether the request in `row` has ended
    take(row) -> result       the ended request's result; the row is free afterwards

DecodeEngine (through the adapter of UniMoEAudio.serve) is one; tests/test_serve_cpu.py drives a fake whose request lengths are known.
"""
from __future__ import annotations

import weakref
from collections import OrderedDict, deque
from typing import Any, Callable, Deque, Dict, Iterable, Iterator, List, NamedTuple, Optional, Sequence, Tuple

MAX_SLOTS = 8          # the default ceiling: the rows of the 16-row decode step
MAX_SLOTS_WIDE = 32    # the most a caller may raise it to: the rows of the wide decode step


class Scheduler:
    def __init__(self, engine, slots: int, poll_every: int = 16, max_slots: int = MAX_SLOTS):
        if not 1 <= max_slots <= MAX_SLOTS_WIDE:
            raise ValueError(f"max_slots must be 1..{MAX_SLOTS_WIDE} (got {max_slots})")
        if not 1 <= slots <= max_slots:
            raise ValueError(f"slots must be 1..{max_slots} (got {slots})")
        if poll_every < 1:
            raise ValueError("poll_every must be >= 1")
        self.engine, self.slots, self.poll_every = engine, int(slots), int(poll_every)
        self.queue: Deque[Tuple[int, Any]] = deque()
        self.free: List[int] = list(range(self.slots))     # ascending: the lowest free row takes the next request
        self.live: Dict[int, int] = {}                      # row -> index of the request it holds
        self.steps_run = 0
        self.admitted: List[Tuple[int, int, int]] = []      # (request index, row, step count at admission), in admission order

    def _admit_free_rows(self, source: Iterator[Tuple[int, Any]]):
        while self.free:
            if not self.queue:
                nxt = next(source, None)
                if nxt is None:
                    return
                self.queue.append(nxt)
            index, request = self.queue.popleft()
            row = self.free.pop(0)
            self.engine.admit(row, request)
            self.live[row] = index
            self.admitted.append((index, row, self.steps_run))

    def run(self, requests: Iterable[Any], hook: Optional[Callable[[Any], Optional[Iterable[Any]]]] = None) -> Iterator[Tuple[int, Any]]:
        """Serves every request of `requests` (any iterable, read lazily: one request ahead of the free rows) and yields
        (index, result) as each ends, index = the request's position in `requests`.
        hook(state), when given, runs at every poll: behind poll(), before any take() of that poll and before the next admission, so
        whatever it reads of a row that has ended (its last frames in the token buffer) is still the ended request's.  What it returns
        (an iterable, or None) is yielded as it is, ahead of the poll's ended requests."""
        source = iter(enumerate(requests))
        while True:
            self._admit_free_rows(source)
            if not self.live:
                return
            self.engine.steps(self.poll_every)
            self.steps_run += self.poll_every
            state = self.engine.poll()
            if hook is not None:
                yield from hook(state) or ()
            for row in sorted(self.live):
                if self.engine.row_done(state, row):
                    index = self.live.pop(row)
                    result = self.engine.take(row)
                    self.free.append(row)
                    self.free.sort()
                    yield index, result


class RowFrames(NamedTuple):
    """What one state read makes final in one live row: frames [f0, f1) are new, `complete`: the request has ended and f1 is its
    length, `t_valid`: the token positions of the row written so far (umoe_rvq_from_delayed reads the rest as pad)."""
    row: int
    f0: int
    f1: int
    complete: bool
    t_valid: int


def final_frames(state: Sequence[int], clock: Sequence[Sequence[int]], prefill_steps: Sequence[int], max_delay: int,
                 emitted: Dict[int, int]) -> List[RowFrames]:
    """DecodeEngine.run_stream's rule on per-row clocks.  state: the engine's state words (eos_detected[B], countdown[B], finished[B],
    prefill_step[B], step, ...), clock: {step_off, t_prompt} per row, both of ONE read; emitted: {row: frames handed out so far} of the
    rows that hold a request.  Row b lives at the local step d = step - step_off[b] and has written token positions [0, d + 1):
    frame t is final once its most delayed channel is written, d >= prefill_step + t + max_delay, and it lies before the row's
    length.  A row whose countdown is 0 has ended: its length is finished - prefill_step (DecodeEngine.take), all of it final, and
    it wrote positions up to finished + max_delay.  One record per row of `emitted`, in row order."""
    B = len(prefill_steps)
    step = int(state[4 * B])
    out = []
    for b in sorted(emitted):
        d = step - int(clock[b][0])
        fin, ps = int(state[2 * B + b]), int(prefill_steps[b])
        length = None if fin == -1 else max(fin - ps, 0)
        complete = int(state[B + b]) == 0 and length is not None
        f1 = max(d + 1 - max_delay - ps, 0)
        if length is not None:
            f1 = length if complete else min(f1, length)
        out.append(RowFrames(b, int(emitted[b]), max(f1, int(emitted[b])), complete, fin + max_delay if complete else d + 1))
    return out


class VoicePrompt:
    """What every request in one voice shares (UniMoEAudio.voice): the reference audio's codes as the codec gave them
    (`codec`) and as the prompt takes them (`pc`, preprocess_codec), the token ids of the prompt up to and including <|SPEECH_START|>
    (`ids`), their embeddings (`x` [len(ids), D]) and, per engine object and prefix length, the prefix store an admission installs.
    Plain host bookkeeping: the tensors are whatever the caller put in."""

    def __init__(self, prompt_transcription: str, codec=None, pc=None, ids=(), x=None):
        self.prompt_transcription = prompt_transcription
        self.codec, self.pc, self.ids, self.x = codec, pc, [int(i) for i in ids], x
        self.stores: Dict[Tuple[int, int], Any] = {}        # (id(engine), P) -> (weak reference to the engine, store)

    def store_for(self, engine, P: int, build: Callable[[int], Any]) -> Tuple[Any, bool]:
        """(the store of the first P prefix tokens on `engine`, whether it was there already); build(P) makes it on a miss"""
        key = (id(engine), int(P))
        held = self.stores.get(key)
        hit = held is not None and held[0]() is engine       # (an id may come back with another engine object)
        if not hit:
            self.stores = {k: v for k, v in self.stores.items() if v[0]() is not None}      # stores of engines that are gone
            self.stores[key] = (weakref.ref(engine), build(int(P)))
        return self.stores[key][1], hit

    def drop(self):
        self.stores.clear()


class VoiceLRU:
    """The voices serve(prefix_cache=True) keeps: at most `cap`, the least recently used dropped first (with its stores)."""

    def __init__(self, cap: int = 8):
        if cap < 1:
            raise ValueError(f"prefix_cache_voices must be >= 1 (got {cap})")
        self.cap = int(cap)
        self.voices: "OrderedDict[Any, VoicePrompt]" = OrderedDict()
        self.evicted = 0

    def get(self, key, make: Callable[[], VoicePrompt]) -> VoicePrompt:
        if key in self.voices:
            self.voices.move_to_end(key)
            return self.voices[key]
        v = self.voices[key] = make()
        while len(self.voices) > self.cap:
            _, old = self.voices.popitem(last=False)
            old.drop()
            self.evicted += 1
        return v


def makespan_steps(lengths: Iterable[int], slots: int, poll_every: int, max_slots: int = MAX_SLOTS) -> int:
    """Decode steps Scheduler.run takes for requests that need `lengths` steps each, in queue order: a request admitted at step a
    is seen ended at the first poll at or after a + length."""
    sched = Scheduler(_Lengths(), slots, poll_every, max_slots)
    for _ in sched.run(list(lengths)):
        pass
    return sched.steps_run


class _Lengths:
    """the engine of makespan_steps: a request IS its length in steps"""

    def __init__(self):
        self.left: Dict[int, int] = {}

    def admit(self, row, request):
        self.left[row] = int(request)

    def steps(self, n):
        for r in self.left:
            self.left[r] -= n

    def poll(self):
        return self.left

    def row_done(self, state, row):
        return state[row] <= 0

    def take(self, row):
        return self.left.pop(row)
