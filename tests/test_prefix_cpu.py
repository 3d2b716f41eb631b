"""CPU suite of prefix reuse across admissions: the host plan of a split admission against a brute-force restatement, the
longest-common-prefix / clamp logic of the API, hit / miss accounting and the LRU cap under the Scheduler, and the two new entries in
the header and the built library.  No device, no compute calls."""
import ctypes
import os
import re
import types

import pytest

from conftest import ROOT

PADS = [(0, 0), (3, 0), (0, 3), (70, 0), (0, 66)]          # the last two: a pad larger than every P below
PS = (1, 5, 63, 64, 65)
TQS = (2, 15, 16, 17)


def _mask(T, pads):
    return [[0] * p + [1] * (T - p) for p in pads]


def brute_force(valid, P):
    """The one-shot rule per slot, restated without the plan's arithmetic: slot t of row r is a pad, or holds the row's token
    i = (valid tokens before t); a prefix token i < P in a slot below P is what the store provides (installed), every slot from P on is
    computed.  Positions: cumsum(mask) - 1, masked -> 1."""
    T = len(valid[0])
    kinds, pos = [], []
    for row in valid:
        k, p, cnt = [], [], 0
        for t in range(T):
            cnt += row[t]
            p.append(cnt - 1 if row[t] else 1)
            if t >= P:
                k.append(("computed", None))
            elif not row[t]:
                k.append(("pad", None))
            else:
                k.append(("installed", cnt - 1))           # the store token this slot must receive
        kinds.append(k)
        pos.append(p)
    return kinds, pos


def covered(plan):
    """what the plan does to every slot below T of every row: a list of labels per slot (exactly one is the requirement)"""
    out = []
    for r in range(len(plan.first)):
        slots = [[] for _ in range(plan.T)]
        for t in range(min(plan.first[r], plan.P)):
            slots[t].append(("pad", None))
        i0, s0, n = plan.install[r]
        for k in range(n):
            slots[s0 + k].append(("installed", i0 + k))
        for j, s in enumerate(plan.kv_pos[r]):
            slots[s].append(("computed", None))
        out.append(slots)
    return out


def check_plan(plan, valid, P):
    """every slot exactly once and as the brute force says, positions the one-shot rule's, queries behind P cached keys"""
    kinds, pos = brute_force(valid, P)
    got = covered(plan)
    for r in range(len(valid)):
        for t in range(plan.T):
            assert len(got[r][t]) == 1, (r, t, got[r][t])
            assert got[r][t][0] == kinds[r][t], (r, t, got[r][t], kinds[r][t])
        assert plan.pos3[r] == pos[r][P:], r
        assert plan.kv_pos[r] == list(range(P, plan.T)), r
        assert plan.q_pos0[r] == P, r
        assert plan.valid_count[r] == sum(valid[r]), r
        assert plan.first[r] == valid[r].index(1), r


@pytest.mark.parametrize("pads", PADS)
def test_prefix_plan_against_brute_force(pads):
    from unimoe_audio_amd.prefix_plan import prefix_plan
    n = 0
    for P in PS:
        for Tq in TQS:
            T = P + Tq
            if max(pads) >= T:
                continue
            valid = _mask(T, pads)
            check_plan(prefix_plan(valid, P), valid, P)
            n += 1
    assert n >= 8, n
    if max(pads) > max(PS):                                  # a pad larger than P: nothing to install in that row
        T = 65 + 17
        plan = prefix_plan(_mask(T, pads), 65)
        r = pads.index(max(pads))
        assert plan.install[r][2] == 0 and plan.install[1 - r] == (0, 0, 65)


def test_planted_errors_are_rejected():
    from unimoe_audio_amd.prefix_plan import prefix_plan
    valid = _mask(64 + 16, (3, 0))
    plan = prefix_plan(valid, 64)
    check_plan(plan, valid, 64)
    i0, s0, n = plan.install[0]
    with pytest.raises(AssertionError):                      # an install shifted by one slot
        check_plan(plan._replace(install=[(i0, s0 + 1, n), plan.install[1]]), valid, 64)
    with pytest.raises(AssertionError):                      # ... or by one store token
        check_plan(plan._replace(install=[(i0 + 1, s0, n - 1), plan.install[1]]), valid, 64)
    with pytest.raises(AssertionError):                      # queries that do not see the cached keys
        check_plan(plan._replace(q_pos0=[0, 0]), valid, 64)
    with pytest.raises(AssertionError):                      # positions that restart behind the prefix
        check_plan(plan._replace(pos3=[[p - 64 for p in row] for row in plan.pos3]), valid, 64)


def test_prefix_plan_refusals():
    from unimoe_audio_amd._lib import UmoeError
    from unimoe_audio_amd.prefix_plan import prefix_plan
    with pytest.raises(UmoeError, match="1 <= P"):
        prefix_plan(_mask(10, (0, 0)), 0)
    with pytest.raises(UmoeError, match="2 <= T - P"):
        prefix_plan(_mask(10, (0, 0)), 9)
    with pytest.raises(UmoeError, match="left-padded"):
        prefix_plan([[1, 0, 1, 1, 1, 1], [1] * 6], 2)
    with pytest.raises(UmoeError, match="no valid token"):
        prefix_plan([[0] * 6, [1] * 6], 2)


class Tok:
    """a stand-in tokenizer: special tokens are one id each, every other character one id; left padding"""

    def __call__(self, texts, add_special_tokens=False, return_tensors="pt", padding=True):
        rows = []
        for t in texts:
            ids = []
            for piece in re.split(r"(<\|[A-Za-z_]+\|>)", t):
                if piece.startswith("<|"):
                    ids.append(300 if piece == "<|AUDIO_PLACEHOLDER|>" else 200 + sum(map(ord, piece)) % 90)
                else:
                    ids += [1 + ord(ch) % 190 for ch in piece]
            rows.append(ids)
        T = max(map(len, rows))
        return types.SimpleNamespace(input_ids=[[0] * (T - len(r)) + r for r in rows], attention_mask=[[0] * (T - len(r)) + [1] * len(r) for r in rows])


def test_split_point_is_the_common_prefix_clamped():
    from unimoe_audio_amd.prefix_plan import common_prefix_len, split_point
    assert common_prefix_len([1, 2, 3], [1, 2, 4], [1, 2, 3, 9]) == 2
    assert common_prefix_len([1, 2], [1, 2], [1, 2]) == 2 and common_prefix_len([5], [6], [5]) == 0
    # the API's texts: prefix up to and including <|SPEECH_START|>, then the sentence (positive row only), then the tail
    head = "<|im_start|>user\n<|SPEECH_PROMPT_START|>hi<|SPEECH_PROMPT_END|><|VOICE_PROMPT_START|>" + "<|AUDIO_PLACEHOLDER|>" * 7 + "<|VOICE_PROMPT_END|><|SPEECH_START|>"
    tail = "<|SPEECH_END|><|im_end|>\n<|AUDIO_START|>"
    tok = Tok()
    voice = tok([head]).input_ids[0]
    enc = tok([head + tail, head + "some words" + tail])
    rows = [[i for i, m in zip(ids, am) if m] for ids, am in zip(enc.input_ids, enc.attention_mask)]
    T = len(enc.input_ids[0])
    assert split_point(rows[0], rows[1], voice, T) == len(voice)             # everything up to and including <|SPEECH_START|>
    assert rows[0][len(voice)] != rows[1][len(voice)]
    # another voice's ids share only the text in front of the transcription
    other = tok([head.replace("hi", "ho")]).input_ids[0]
    assert 0 < split_point(rows[0], rows[1], other, T) < len(voice) - 7
    # the clamp: the engine runs at least two columns behind the prefix
    same = list(range(1, 21))
    assert split_point(same, same, same, 20) == 18
    assert split_point(same[:1], same[:1], same, 1) == -1                    # nothing to split: the caller admits in one piece


class FakeEngine:
    """the engine side of Scheduler, with the hit / miss bookkeeping serve() does: requests are (voice key, steps)"""

    def __init__(self, cap):
        from unimoe_audio_amd.serve import VoiceLRU
        self.voices, self.left, self.log, self.built, self.made = VoiceLRU(cap), {}, [], 0, 0

    def _make(self, key):
        from unimoe_audio_amd.serve import VoicePrompt
        self.made += 1
        return VoicePrompt(key, ids=[1, 2, 3])

    def _build(self, P):
        self.built += 1
        return ("store", P)

    def admit(self, row, request):
        key, steps = request
        voice = self.voices.get(key, lambda: self._make(key))
        store, hit = voice.store_for(self, 3, self._build)
        assert store == ("store", 3)
        self.log.append((key, hit))
        self.left[row] = steps

    def steps(self, n):
        for r in self.left:
            self.left[r] -= n

    def poll(self):
        return self.left

    def row_done(self, state, row):
        return state[row] <= 0

    def take(self, row):
        return self.left.pop(row)


def test_scheduler_hit_miss_accounting_and_lru_cap():
    from unimoe_audio_amd.serve import Scheduler, VoicePrompt
    reqs = [("a", 4), ("b", 4), ("a", 4), ("a", 8), ("b", 4), ("a", 4)]
    eng = FakeEngine(cap=8)
    done = [i for i, _ in Scheduler(eng, 4, poll_every=4).run(reqs)]
    assert sorted(done) == list(range(6))
    assert [h for _, h in eng.log] == [False, False, True, True, True, True]      # 2 misses, 4 hits
    assert eng.built == 2 and eng.made == 2
    # cap 2, three voices: a's hit makes b the least recently used, so c evicts b; b then evicts a, a evicts c -- each builds again
    eng = FakeEngine(cap=2)
    seq = [("a", 1), ("b", 1), ("a", 1), ("c", 1), ("b", 1), ("a", 1)]
    for _ in Scheduler(eng, 1, poll_every=1).run(seq):
        pass
    assert [h for _, h in eng.log] == [False, False, True, False, False, False], eng.log
    assert eng.voices.evicted == 3 and len(eng.voices.voices) == 2
    # another engine object never sees this engine's stores
    v = VoicePrompt("x", ids=[1])
    e1, e2 = FakeEngine(1), FakeEngine(1)
    assert v.store_for(e1, 1, e1._build)[1] is False and v.store_for(e1, 1, e1._build)[1] is True
    assert v.store_for(e2, 1, e2._build)[1] is False and v.store_for(e1, 2, e1._build)[1] is False
    with pytest.raises(ValueError):
        FakeEngine(0)


def test_prefix_entries_are_declared_and_exported():
    from unimoe_audio_amd import _lib
    txt = open(os.path.join(ROOT, "include", "umoe.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = ctypes.CDLL(_lib.build())
    for name in ("umoe_engine_prefix_build", "umoe_engine_admit_prefix", "umoe_kv_prefix_copy"):
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
    assert len(_lib.lib().umoe_engine_admit_prefix.argtypes) == 11 and len(_lib.lib().umoe_engine_prefix_build.argtypes) == 7
