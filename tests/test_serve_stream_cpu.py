"""CPU suite of streamed serving: which frames are final on per-row clocks (serve.final_frames) against a host restatement of
umoe_delay_step_clock, the per-row DAC decoder's schedule run by the float64 restatement of tests/test_dac_stream_cpu.py against a
float64 full decode, planted errors, the scheduler's per-poll hook, and the ABI surface (symbols, the table layouts of umoe.h)."""
import os
import random
import re

import pytest
import torch

from conftest import ROOT
from tests.test_dac_stream_cpu import Stream64, _full_decode64, _tiny
from tests.test_serve_cpu import FakeEngine

NEW_SYMBOLS = ["umoe_dac_conv1d_win_rows", "umoe_dac_conv_transpose1d_win_rows", "umoe_dac_shift_rows", "umoe_rvq_from_delayed_rows"]
DELAY = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]
MD = max(DELAY)


# ---------------------------------------------------------------------------------------------------- finality
class ClockSim:
    """The scalar half of umoe_delay_step_clock restated on the host: eos_detected, countdown, finished per row, the step word, and
    which token positions each row has written.  eos_at[b]: the local positions `cur` at which row b's channel 0 samples EOS."""

    def __init__(self, B):
        self.B = B
        self.state = [0] * B + [0] * B + [-1] * B + [1] * B + [0, 0, 1, 0, 0, 0, 0, 0]
        self.clock = [[0, 0] for _ in range(B)]
        self.max_tokens = [0] * B
        self.eos_at = [set() for _ in range(B)]
        self.written = [set() for _ in range(B)]

    def admit(self, b, prefill_step, max_tokens, eos_at=()):
        B, st = self.B, self.state
        self.clock[b] = [st[4 * B] - (prefill_step - 1), 7]          # row_admit_kernel
        st[b], st[B + b], st[2 * B + b], st[3 * B + b] = 0, -1, -1, prefill_step
        self.max_tokens[b], self.eos_at[b] = max_tokens, set(eos_at)
        self.written[b] = set(range(prefill_step))                   # the request's own prefix

    def step(self):
        B, st = self.B, self.state
        if all(st[B + b] == 0 for b in range(B)):
            return
        dec_step = st[4 * B]
        for b in range(B):
            cd = st[B + b]
            active = cd != 0
            cur = dec_step - self.clock[b][0] + 1
            trig = active and ((not st[b] and cur in self.eos_at[b]) or cur >= self.max_tokens[b] - MD)
            if trig:
                st[b] = 1
            if trig and cd < 0:
                st[B + b], st[2 * B + b] = MD, cur
            if st[B + b] > 0:
                st[B + b] -= 1
            if active:
                self.written[b].add(cur)
        st[4 * B] = dec_step + 1


def _check_frames(sim, frames, emitted):
    """what final_frames may claim, from the simulated rows alone"""
    B = sim.B
    for fr in frames:
        b, ps = fr.row, sim.state[3 * B + fr.row]
        assert fr.f0 == emitted[b] and fr.f1 >= fr.f0
        # the row wrote exactly the positions below t_valid
        assert sim.written[b] == set(range(fr.t_valid)), (b, fr)
        # every channel of every final frame is written ...
        assert all(ps + t + d < fr.t_valid for t in range(fr.f0, fr.f1) for d in DELAY), (b, fr)
        ended = sim.state[B + b] == 0
        assert fr.complete == ended
        length = None if sim.state[2 * B + b] == -1 else max(sim.state[2 * B + b] - ps, 0)
        if ended:
            assert fr.f1 == length                                  # DecodeEngine.take()'s
        else:
            # ... and no frame that is written through and inside the row's length is held back
            nxt = fr.f1
            assert not (ps + nxt + MD < fr.t_valid and (length is None or nxt < length)), (b, fr)


def test_final_frames_on_rows_at_different_offsets():
    from unimoe_audio_amd.serve import final_frames
    sim = ClockSim(5)
    emitted = {}
    sim.admit(0, prefill_step=1, max_tokens=200, eos_at={30})       # ends by EOS
    sim.admit(1, prefill_step=3, max_tokens=40)                     # ends by its own max_tokens
    emitted.update({0: 0, 1: 0})
    seen = {b: [] for b in range(5)}
    for poll in range(8):
        if poll == 2:
            sim.admit(2, prefill_step=2, max_tokens=300)            # a later admission: another offset
            emitted[2] = 0
        for _ in range(8):
            sim.step()
        if poll == 4:
            sim.admit(4, prefill_step=1, max_tokens=100)            # admitted at this very poll: local step 0, nothing final
            emitted[4] = 0
        frames = final_frames(sim.state, sim.clock, sim.state[15:20], MD, emitted)      # row 3 is parked throughout: not in `emitted`
        assert [fr.row for fr in frames] == sorted(emitted)
        _check_frames(sim, frames, emitted)
        for fr in frames:
            seen[fr.row].append((fr.f0, fr.f1, fr.complete))
            emitted[fr.row] = fr.f1
            if fr.complete:
                del emitted[fr.row]
        if poll == 4:
            assert seen[4] == [(0, 0, False)]
    assert seen[0][-1] == (seen[0][-1][0], 30 - 1, True) and seen[1][-1][1:] == (40 - MD - 3, True)
    assert not seen[3] and seen[2][-1][2] is False and seen[2][-1][1] > 0
    assert len({tuple(c) for c in sim.clock[:3]}) == 3              # three rows on three clocks


def _run_stream_rule(st, B, ps, emitted, complete, over):
    """DecodeEngine.run_stream's loop body on one read of the state words"""
    dec_step, rows = int(st[4 * B]), []
    for b in range(B):
        if complete[b]:
            continue
        fin = int(st[2 * B + b])
        if over:
            final_len = max((dec_step + 1 - MD if fin == -1 else fin) - ps[b], 0)
        else:
            final_len = None if fin == -1 else max(fin - ps[b], 0)
        f1 = max(dec_step + 1 - MD - ps[b], 0)
        if final_len is not None:
            f1 = final_len if over else min(f1, final_len)
        complete[b] = final_len is not None and f1 == final_len
        if f1 > emitted[b] or complete[b]:
            rows.append((b, emitted[b], f1, complete[b]))
            emitted[b] = f1
    return rows


@pytest.mark.parametrize("chunk", [1, 7, 25])
def test_final_frames_at_offset_zero_is_run_streams_rule(chunk):
    from unimoe_audio_amd.serve import final_frames
    B, ps = 3, [1, 1, 1]
    sim = ClockSim(B)
    for b, (mx, eos) in enumerate([(90, {20}), (60, ()), (120, {45, 50})]):
        sim.admit(b, 1, mx, eos)
    assert all(c[0] == 0 for c in sim.clock)
    em_a, done_a = [0] * B, [False] * B
    em_b = {b: 0 for b in range(B)}
    while not all(done_a):
        for _ in range(chunk):
            sim.step()
        over = all(sim.state[B + b] == 0 for b in range(B))
        want = _run_stream_rule(sim.state, B, ps, em_a, done_a, over)
        got = []
        for fr in final_frames(sim.state, sim.clock, ps, MD, em_b):
            if fr.f1 > fr.f0 or fr.complete:
                got.append((fr.row, fr.f0, fr.f1, fr.complete))
            em_b[fr.row] = fr.f1
            if fr.complete:
                del em_b[fr.row]
        assert got == want, (sim.state[4 * B], got, want)
    assert not em_b


def _codes(tokens, ps, f0, f1, t_valid, pad):
    """umoe_rvq_from_delayed's read of frames [f0, f1) of one row: tokens[ps + t + delay_c][c], the pad code at or past t_valid"""
    return [[tokens[ps + t + d][c] if ps + t + d < t_valid else pad for c, d in enumerate(DELAY)] for t in range(f0, f1)]


def test_a_t_valid_taken_from_another_row_is_caught():
    """two rows on different clocks: with each row's own t_valid the streamed codes are those of the finished request; with the
    t_valid of the row that is behind, the other row's newest frames read as pad"""
    from unimoe_audio_amd.serve import final_frames
    rng = random.Random(0)
    sim = ClockSim(2)
    sim.admit(0, 1, 200)
    for _ in range(16):
        sim.step()
    sim.admit(1, 1, 200)
    for _ in range(24):
        sim.step()
    tokens = [[[rng.randrange(1024) for _ in DELAY] for _ in range(260)] for _ in range(2)]
    frames = {fr.row: fr for fr in final_frames(sim.state, sim.clock, [1, 1], MD, {0: 0, 1: 0})}
    assert frames[0].t_valid == frames[1].t_valid + 16 and frames[0].f1 > frames[1].f1 > 0
    full = lambda b: _codes(tokens[b], 1, frames[b].f0, frames[b].f1, 260, -7)          # noqa: E731  (every position valid)

    def check(t_valid_of):
        for b in (0, 1):
            assert _codes(tokens[b], 1, frames[b].f0, frames[b].f1, frames[t_valid_of[b]].t_valid, -7) == full(b), b

    check({0: 0, 1: 1})
    with pytest.raises(AssertionError):
        check({0: 1, 1: 1})


# ---------------------------------------------------------------------------------------------------- the per-row decoder in float64
def _rows64(base):
    class Rows64(base):
        """DacRowStreamDecoder's bookkeeping and slabs; every window computed in float64 from the slab contents only"""

        def __init__(self, model, slots, ragged, max_frames=25):
            self.z = {}                                    # row -> latents [Dl, T] of the sequence it holds
            super().__init__(model, slots, self._src, max_frames=max_frames, ragged=ragged, dtype=torch.float64, device=torch.device("cpu"))
            for b in self.bufs:
                b.fill_(float("nan"))
            self.windows, self.wlog, self.calls = [], [], 0      # (windows: Stream64._conv's own log)

        def _src(self, requests, slab):
            for row, f0, n, col in requests:
                assert f0 + n <= self.z[row].shape[1]
                slab[row, :, col:col + n] = self.z[row][:, f0:f0 + n]

        def _upload(self, host):
            return host

        def _shift(self, i, moves, table=None):
            self.calls += 1
            for r, shift, count in moves:
                self.bufs[i][r, :, :count] = self.bufs[i][r, :, shift:shift + count].clone()
                self.bufs[i][r, :, count:] = float("nan")  # nothing behind the kept context may be read before it is written

        def _conv(self, ly, x, x_off, L_true, t0, n, resid, r_off, y, y_off):
            self.calls += 1
            Stream64._conv(self, ly, x, x_off, L_true, t0, n, resid, r_off, y, y_off)

        def _conv_rows(self, i, wins, wave, table):
            self.calls += 1
            host = table[0]
            assert host.shape == (self.slots, 12)
            for v in wins:
                x, resid, y = self._planes(i, v, wave)
                # the table row says what the window record says
                assert host[v.slot].tolist() == [x.data_ptr(), 0 if resid is None else resid.data_ptr(), y.data_ptr(), v.x_off, x.shape[2], v.r_off,
                                                 0 if resid is None else resid.shape[2], v.y_off, y.shape[2], v.t0, v.n, v.L_true]
                Stream64._conv(self, self.plan.layers[i], x, v.x_off, v.L_true, v.t0, v.n, resid, v.r_off, y, v.y_off)
            idle = [r for r in range(self.slots) if r not in {v.slot for v in wins}]
            assert all(int(host[r, 10]) == 0 for r in idle)
    return Rows64


# (push per row; "F2" flushes row 2, "R2" resets it): rows start at different pushes, push 1, 7, 16 or 25 frames, row 1 is idle in some
# pushes, row 2 is flushed, reset and reused for a second sequence
SCHEDULE = [[7, 0, 0], [25, 1, 0], [1, 0, 16], [16, 7, 25], [7, 0, 1], "F2", "R2", [1, 16, 7], [0, 25, 25], [25, 0, 16], [16, 1, 0], "F0", [0, 7, 1], "F1",
            "F2"]


def _drive(dec, model, seed=0, schedule=SCHEDULE, reset=None):
    """runs the schedule -> {(row, sequence number): (samples, latents)}, and checks the windows tile every layer's [0, L)"""
    g = torch.Generator().manual_seed(seed)
    slots = dec.slots
    seq, pushed, got, out = [0] * slots, [0] * slots, {}, {}
    total = {}
    for r in range(slots):                                 # how many frames each sequence gets, up to its flush
        k = 0
        total[(r, 0)] = 0
        for ev in schedule:
            if isinstance(ev, str):
                k += ev == f"R{r}"
                total.setdefault((r, k), 0)
            else:
                total[(r, k)] += ev[r]
    lat = {key: torch.randn(model.latent_dim, n, dtype=torch.float64, generator=g) for key, n in total.items() if n}
    dec.z = {r: lat[(r, 0)] for r in range(slots) if (r, 0) in lat}
    for ev in schedule:
        if isinstance(ev, str):
            r = int(ev[1])
            if ev[0] == "F":
                got.setdefault((r, seq[r]), []).append(dec.flush([r])[r].clone())
                out[(r, seq[r])] = (torch.cat(got[(r, seq[r])]), lat[(r, seq[r])][:, :pushed[r]])
            else:
                (reset or dec.reset)(r)
                seq[r], pushed[r] = seq[r] + 1, 0
                dec.z[r] = lat[(r, seq[r])]
            continue
        mark = len(dec.wlog)
        for r, a in dec.push(ev).items():
            got.setdefault((r, seq[r]), []).append(a.clone())
        assert all(ev[w[1]] > 0 for w in dec.wlog[mark:])          # an idle row computes nothing
        pushed = [p + n for p, n in zip(pushed, ev)]
    return out


def _with_window_log(cls):
    class Logged(cls):
        def _execute(self, work, wave):
            for i, wins in enumerate(work["conv"]):
                self.wlog.extend((i, v.slot, v.t0, v.n, v.L_true, v.x_off, v.r_off, v.y_off) for v in wins)
            super()._execute(work, wave)
    return Logged


@pytest.mark.parametrize("rates", [(8, 5, 4, 2), (3, 2)])
def test_row_decoder_matches_full_decode_float64(rates):
    from unimoe_audio_amd.dac import DacRowStreamDecoder, stream_plan
    model = _tiny(rates)
    plan = stream_plan(model)
    Rows64 = _with_window_log(_rows64(DacRowStreamDecoder))
    logs, calls = {}, {}
    for ragged in (True, False):
        dec = Rows64(model, 3, ragged)
        res = _drive(dec, model)
        assert sorted(res) == [(0, 0), (1, 0), (2, 0), (2, 1)]
        for key, (wave, z) in res.items():
            ref = _full_decode64(model, z[None])[0]
            assert wave.shape[0] == plan.out_len(z.shape[1]) == ref.shape[0], key
            assert torch.allclose(wave, ref, rtol=0, atol=1e-12), (key, (wave - ref).abs().max())
        logs[ragged], calls[ragged] = dec.wlog, dec.calls
        assert dec.grown == 0
        # per layer and row the windows tile [0, L) of every sequence: each starts where the last ended, none is empty, and the last
        # ends at the layer's true output length
        for r in range(3):
            for i, ly in enumerate(plan.layers):
                ws = [w for w in dec.wlog if w[0] == i and w[1] == r]
                ends, pos = [], 0
                for _, _, t0, n, *_ in ws:
                    assert n > 0
                    if t0 == 0 and pos:
                        ends.append(pos)                   # the row was reset: a new sequence
                        pos = 0
                    assert t0 == pos, (i, r, t0, pos)
                    pos += n
                ends.append(pos)
                lens = []
                for key in sorted(k for k in res if k[0] == r):
                    L = res[key][1].shape[1]
                    for lj in plan.layers[:i + 1]:
                        L = lj.out_len(L)
                    lens.append(L)
                assert ends == lens, (i, r, ends, lens)
    # the grouped and the ragged executor are handed identical windows per row
    assert logs[True] == logs[False]
    # ragged: the calls of a push do not depend on what the rows do: one per buffer (moves) and one per layer
    n_events = len(SCHEDULE) - sum(ev[0] == "R" for ev in SCHEDULE if isinstance(ev, str))
    assert calls[True] == n_events * 2 * len(plan.layers) and calls[False] != calls[True]


# one row; three rows that part (tests/test_dac_stream_cpu.py's schedule): (pushes per row, the flushes that end it)
SHARED = {"one_row": ([[1], [7], [25], [1], [25], [2]], [[0]]),
          "rows_part": ([[1, 1, 1], [7, 7, 7], [25, 25, 25], [1, 7, 7], [25, 1, 0], [2, 20, 0]], [[2], [0, 1]])}


@pytest.mark.parametrize("name", sorted(SHARED))
@pytest.mark.parametrize("rates", [(8, 5, 4, 2), (3, 2)])
def test_grouped_and_row_decoder_run_one_schedule(rates, name):
    """DacStreamDecoder and DacRowStreamDecoder on the same pushes and flushes (min_duration=1): every row is handed the same windows
    (layer, t0, n, L_true, x_off, r_off, y_off) in the same order, and its samples are equal bit for bit"""
    from unimoe_audio_amd.dac import DacRowStreamDecoder
    pushes, flushes = SHARED[name]
    model = _tiny(rates)
    B = len(pushes[0])
    z = torch.randn(B, model.latent_dim, max(sum(ev[r] for ev in pushes) for r in range(B)), dtype=torch.float64,
                    generator=torch.Generator().manual_seed(3))

    class Grouped(Stream64):
        def _conv(self, ly, x, x_off, L_true, t0, n, resid, r_off, y, y_off):
            i = self.plan.layers.index(ly)
            g = next(g for g in self._groups if g.bufs[i] is x)
            self.wlog.extend((i, r, t0, n, L_true, x_off, r_off, y_off) for r in g.rows)
            super()._conv(ly, x, x_off, L_true, t0, n, resid, r_off, y, y_off)

    grouped, rows = Grouped(model, B, z), _with_window_log(_rows64(DacRowStreamDecoder))(model, B, True)
    grouped.wlog, rows.z = [], {r: z[r] for r in range(B)}
    got = {id(dec): [[] for _ in range(B)] for dec in (grouped, rows)}
    for dec in (grouped, rows):
        for ev in pushes:
            for r, a in dec.push(ev).items():
                got[id(dec)][r].append(a.clone())
        for ends in flushes:
            for r, a in dec.flush(ends, min_duration=1).items():
                got[id(dec)][r].append(a.clone())
    for r in range(B):
        mine = [w for w in grouped.wlog if w[1] == r]
        assert mine and mine == [w for w in rows.wlog if w[1] == r], r
        a, b = torch.cat(got[id(grouped)][r]), torch.cat(got[id(rows)][r])
        n, sr = grouped.plan.out_len(sum(ev[r] for ev in pushes)), model.sample_rate
        assert a.shape[0] == n + (int((1 - n / sr) * sr) if n < sr else 0) and torch.equal(a, b), r


def test_flush_pads_like_dac_decode_and_reset_reopens_the_row():
    from unimoe_audio_amd.dac import DacRowStreamDecoder, stream_plan
    model = _tiny()
    dec = _rows64(DacRowStreamDecoder)(model, 2, True)
    dec.z = {1: torch.randn(model.latent_dim, 12, dtype=torch.float64)}
    a = dec.push([0, 12]).get(1)
    b = dec.flush(1, min_duration=1)[1]
    n, sr = stream_plan(model).out_len(12), model.sample_rate
    assert a.shape[0] + b.shape[0] == n + int((1 - n / sr) * sr)
    assert torch.count_nonzero(b[b.shape[0] - int((1 - n / sr) * sr):]) == 0
    with pytest.raises(ValueError):
        dec.push([0, 1])
    dec.reset(1)
    dec.z[1] = torch.randn(model.latent_dim, 3, dtype=torch.float64)
    dec.push([0, 3])


def test_a_reset_that_keeps_the_old_have_is_caught():
    from unimoe_audio_amd.dac import DacRowStreamDecoder, _Timeline
    model = _tiny((3, 2))
    Rows64 = _with_window_log(_rows64(DacRowStreamDecoder))

    def run(planted):
        dec = Rows64(model, 3, True)

        def bad_reset(r):
            old = dec.rows[r]
            dec.rows[r] = _Timeline(len(dec.plan.layers))
            dec.rows[r].have = list(old.have)

        res = _drive(dec, model, reset=bad_reset if planted else None)
        wave, z = res[(2, 1)]
        ref = _full_decode64(model, z[None])[0]
        assert wave.shape == ref.shape and torch.allclose(wave, ref, rtol=0, atol=1e-12)

    run(False)
    with pytest.raises(AssertionError):
        run(True)


def _plant_trimmed_context(monkeypatch):
    """the plant, in the one schedule both decoders run: every timeline made from here on trims buffer 0 one position too far"""
    from unimoe_audio_amd import dac as D

    class Trimmed(D._Timeline):
        def windows(self, plan, final, room):
            yield from super().windows(plan, final, room)
            if self.keep[0] < self.have[0]:
                self.keep[0] += 1                          # buffer 0 feeds a K = 7 conv: it needs its 3 positions of left context

    monkeypatch.setattr(D, "_Timeline", Trimmed)


def test_left_context_trimmed_one_position_too_far_is_caught(monkeypatch):
    from unimoe_audio_amd.dac import DacRowStreamDecoder
    model = _tiny((3, 2))
    Rows64 = _with_window_log(_rows64(DacRowStreamDecoder))
    _drive(Rows64(model, 3, True), model)
    _plant_trimmed_context(monkeypatch)
    with pytest.raises(AssertionError):
        _drive(Rows64(model, 3, True), model)


def test_left_context_trimmed_one_position_too_far_is_caught_in_the_grouped_decoder(monkeypatch):
    model = _tiny((3, 2))
    z = torch.randn(3, model.latent_dim, 61, dtype=torch.float64)
    pushes, flushes = SHARED["rows_part"]

    class Driven(Stream64):
        def drive(self):
            for ev in pushes:
                self.push(ev)
            for ends in flushes:
                self.flush(ends)
            return self.samples

    assert Driven(model, 3, z).drive() == [Driven(model, 3, z).plan.out_len(n) for n in (61, 61, 40)]
    _plant_trimmed_context(monkeypatch)
    with pytest.raises(AssertionError) as err:
        Driven(model, 3, z).drive()
    # the planted reason: Stream64._conv's (kind, t0, n, first read, last read, x_off, width) says that a window of the K = 7 conv behind
    # buffer 0 reads the one position left of what the decoder kept
    said = re.match(r"\('conv', (\d+), (\d+), (\d+), (\d+), (\d+),", str(err.value))
    assert said, str(err.value)
    t0, n, first, last, x_off = map(int, said.groups())
    assert first == max(t0 - 3, 0) == x_off - 1


# ---------------------------------------------------------------------------------------------------- the scheduler's hook
def _run_as_before(sched, requests):
    """Scheduler.run as it was before it had a hook"""
    source = iter(enumerate(requests))
    while True:
        sched._admit_free_rows(source)
        if not sched.live:
            return
        sched.engine.steps(sched.poll_every)
        sched.steps_run += sched.poll_every
        state = sched.engine.poll()
        for row in sorted(sched.live):
            if sched.engine.row_done(state, row):
                index = sched.live.pop(row)
                result = sched.engine.take(row)
                sched.free.append(row)
                sched.free.sort()
                yield index, result


@pytest.mark.parametrize("slots,poll_every,seed", [(8, 16, 0), (3, 16, 1), (1, 4, 2), (8, 1, 3), (4, 25, 4)])
def test_scheduler_hook_runs_before_take_and_admission(slots, poll_every, seed):
    from unimoe_audio_amd.serve import Scheduler
    rng = random.Random(seed)
    reqs = [(f"r{i}", rng.choice([1, 7, 16, 40, 150, 151, 400, 1000])) for i in range(3 * slots + 5)]
    # hook=None: the sequence and the engine's log are those of the loop as it was
    runs = []
    for how in ("before", "default", "none"):
        eng = FakeEngine(slots)
        sched = Scheduler(eng, slots, poll_every)
        out = list(_run_as_before(sched, iter(reqs)) if how == "before" else sched.run(iter(reqs)) if how == "default" else
                   sched.run(iter(reqs), hook=None))
        runs.append((out, eng.log, sched.admitted, sched.steps_run))
    assert runs[0] == runs[1] == runs[2]
    # a hook: once per poll, with the poll's state, while every row that ended in this poll is still held and not yet taken, and before
    # the next request is admitted into it
    eng = FakeEngine(slots)
    sched = Scheduler(eng, slots, poll_every)
    seen = []

    def hook(state):
        ended = [row for row in sched.live if eng.row_done(state, row)]
        assert all(row in eng.rows for row in ended)                   # not taken yet
        eng.log.append(("hook", eng.clock, tuple(ended), None))
        seen.append(eng.clock)
        return [("chunk", eng.clock, row) for row in ended]

    out = list(sched.run(iter(reqs), hook))
    assert seen == list(range(poll_every, sched.steps_run + 1, poll_every)) and len(seen) == eng.polls
    assert [o for o in out if o[0] != "chunk"] == runs[0][0]
    for k, e in enumerate(eng.log):
        if e[0] != "hook":
            continue
        behind = eng.log[k + 1:]
        nxt = next((j for j, b in enumerate(behind) if b[0] == "hook"), len(behind))
        takes = [b[2] for b in behind[:nxt] if b[0] == "take"]
        assert sorted(takes) == sorted(e[2])                           # exactly the rows the hook saw ended are taken behind it
        for row in e[2]:                                               # and admitted into only behind their take
            evs = [b[0] for b in behind[:nxt] if b[2] == row]
            assert evs in (["take"], ["take", "admit"]), evs
    # what the hook returns is yielded ahead of the poll's results
    pos = {o: k for k, o in enumerate(out)}
    for o in out:
        if o[0] == "chunk":
            name = next(e[3] for e in eng.log if e[0] == "take" and e[1] == o[1] and e[2] == o[2])
            assert pos[o] < pos[(next(i for i, r in enumerate(reqs) if r[0] == name), name)]


# ---------------------------------------------------------------------------------------------------- symbols and tables
def test_new_symbols_and_table_layouts():
    import ctypes
    from unimoe_audio_amd import _lib
    from unimoe_audio_amd import dac as D
    hdr = open(os.path.join(ROOT, "include", "umoe.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.EXPORTS
    assert len(_lib.STRUCT_MIRRORS) == 16
    L = ctypes.CDLL(_lib.build())
    for name in NEW_SYMBOLS:
        assert hasattr(L, name)
    words = {k: int(v) for k, v in re.findall(r"#define (UMOE_(?:DAC|RVQ|SHIFT)_ROW_WORDS) (\d+)", hdr)}
    assert words == {"UMOE_DAC_ROW_WORDS": len(D.DAC_ROW_FIELDS), "UMOE_RVQ_ROW_WORDS": len(D.RVQ_ROW_FIELDS),
                     "UMOE_SHIFT_ROW_WORDS": len(D.SHIFT_ROW_FIELDS)}
    # the comment of umoe.h names the words in the builder's order: "<index> <name>" for every word
    block = hdr[hdr.index("Per-row window tables"):hdr.index("#define UMOE_DAC_ROW_WORDS")]
    for macro, fields in (("UMOE_DAC_ROW_WORDS", D.DAC_ROW_FIELDS), ("UMOE_RVQ_ROW_WORDS", D.RVQ_ROW_FIELDS), ("UMOE_SHIFT_ROW_WORDS", D.SHIFT_ROW_FIELDS)):
        sec = block[block.index(macro):]
        sec = sec[:sec.index("UMOE_", 8)] if "UMOE_" in sec[8:] else sec
        named = [(int(k), n) for k, n in re.findall(r"(?<![\w\[])(\d+) ([A-Za-z_]\w*)", sec)]
        assert named[:len(fields)] == list(enumerate(fields)), (macro, named)
    assert D.dac_row_words(x=5, n=3, L=9) == [5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 9]
    assert D.dac_row_words(**{k: i + 1 for i, k in enumerate(D.DAC_ROW_FIELDS)}) == list(range(1, 13))
