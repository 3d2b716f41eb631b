"""GPU suite of the WP12 form of the wide decode step: umoe_gemm_wide_w12 streams the lossless 12-bit copies of bf16 expert
weights for 17..64 rows, and a bf16 engine of 9 to 32 requests built with w12_wide=True decodes with it.

WP12 holds the bf16 bits, so bit-identity is the only criterion: the kernel against umoe_gemm_wide on the WP16 weights the blocks were packed
from, the engine against the engine without the switch, serving against serving.  No tolerance anywhere: outputs are compared as integers.

Kernel shapes: rows 18 / 32 / 34 / 48 / 64; gate/up at K 2048 (64 k-steps: wave slices of 4 whole 2-step chunks) with n_blocks 12 / 4 / 20
(3, 1 and 5 workgroups of 4 blocks; groups narrower than the grid's box leave early) and once at K 512; down at K 2752 (86 k-steps, even: 2-step chunks), at K 1376
(43, odd: 1-step chunks, slices 0, 5, 10, 16, ...) and with both kinds of group in one launch, n_blocks 3 / 5 / 1 (at two tiles the last
workgroup holds one real block and a clamped copy of it); 1, 3 and 11 groups.  Guards of every run: 0xFF
in the WP12 bytes behind n_blocks, block records behind n_blocks whose entries would patch NaN into k-steps of every wave, and the sentinels
and NaN pad rows of test_gpu_wide_gemm."""
import functools

import pytest
import torch

from test_gpu_wide_gemm import BF16, EPIS, F32, NAN, RESID, ROWS, SENT, SWIGLU, bits, check_fp64, check_guards, make, run_wide
from test_gpu_wide_decode import GREEDY, LMAX, ROW, SAMPLED, T, TMAX, run, serve_run
from test_wide_cpu import wide_wave_steps

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
WV = 8
VALS = [0.0, 2.0 ** -30, 8.0]           # zero, a value far below the window, a value above it: exceptions in N(0, 0.02^2) weights


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ kernel
def plant(W, U, blk32=None):
    """Exceptions in EVERY 16-row block of a row-major weight [N][K]: the first and the last k-step of every wave's K slice (the kernel's
    split for this launch's U: both k-steps of a 2-step chunk, the uneven 0, 5, 10, 16, ... split at 43 k-steps), the K quarter rotating with
    the wave and the block so that lanes of all four quarters carry entries -- 16 per block; block 1 (or the only block) gets two more
    entries in ONE k-step (the patch loop): 18, under the cap with the natural ones (at most 9).  blk32: that block is filled up to exactly
    32 exceptions (the caller checks the count after packing)."""
    from unimoe_audio_amd import w12
    N, K = W.shape
    KB, q = K // 32, K // 4
    n = 0
    for nb in range(N // 16):
        for w, (i0, i1) in enumerate(wide_wave_steps(KB, U, WV)):
            for e, i in enumerate((i0, i1 - 1)):
                h = (w + nb + e) % 4
                W[nb * 16 + (3 * w + 5 * nb + e) % 16, h * q + i * 8 + (2 * w + 7 * e) % 8] = VALS[n % 3]
                n += 1
        if nb == min(1, N // 16 - 1):
            i = wide_wave_steps(KB, U, WV)[3][0] + 1
            W[nb * 16 + 2, 2 * q + i * 8 + 4] = VALS[2]
            W[nb * 16 + 9, 2 * q + i * 8 + 4] = VALS[0]
    if blk32 is not None:
        rows = W[blk32 * 16:blk32 * 16 + 16]
        have = int(w12.exceptions_per_block(w12.pack(w12.wp16_from_rows(rows).view(torch.int16), KB)[1])[0])
        i = wide_wave_steps(KB, U, WV)[5][0] + 1          # (a k-step and element no entry above uses: j = 3 at an odd distance from i0)
        for x in range(32 - have):
            rows[x % 16, (x // 16) * q + i * 8 + 3] = VALS[2]
    return W


def gauss12(name, rows, ks, nbs, seed, planted=False):
    """a case in the layout of test_gpu_wide_gemm.make with the K and n_blocks of every group given: weights N(0, 0.02^2)"""
    epi, waves, u = EPIS[name][:3]
    g = torch.Generator().manual_seed(seed)
    groups = []
    for gi, (k, nb) in enumerate(zip(ks, nbs)):
        N = 8 * nb if epi == SWIGLU else 16 * nb
        A = torch.randn(rows, k, generator=g).to(bf16)
        ws = [(torch.randn(N, k, generator=g) * 0.02).to(bf16) for _ in range(2 if epi == SWIGLU else 1)]
        if planted:
            for j, w in enumerate(ws):
                plant(w, u, blk32=0 if (gi == 0 and j == 0) else None)
        groups.append(dict(k=k, nb=nb, N=N, A=A, w=ws, bias=None, resid=None, planted=planted, full=planted and gi == 0))
    return dict(name=name, epi=epi, waves=waves, u=u, rows=rows, groups=groups, n_valid=16 * max(nbs))


def nan_records(n, KB, dev):
    """`n` block records whose 33 entries, spread over the k-steps of every wave, would patch NaN into the operand"""
    from unimoe_audio_amd import w12
    steps = sorted((x * KB) // 33 for x in range(33))
    ent = [(i << 25) | ((5 * x % 64) << 19) | ((x % 8) << 16) | 0x7FC0 for x, i in enumerate(steps)]
    rec = ent + [0xFFFFFFFF] * (w12.META - 1 - len(ent)) + [0x3C]
    t = torch.tensor([v - (1 << 32) if v >= 1 << 31 else v for v in rec], dtype=torch.int64).to(torch.int32)
    return t.repeat(n).to(dev)


def run_wide_w12(c, dev, call=None):
    """run_wide of test_gpu_wide_gemm on the WP12 copies of the same WP16 packs, every guard in place -> per group the output buffer (with
    its margins)"""
    from unimoe_audio_amd import ops, w12
    rows, epi = c["rows"], c["epi"]
    tiles = (rows + 15) // 16
    ws, ms, bs, outs = [], [], [], []
    ldo = 16 * max(q["nb"] for q in c["groups"]) + 12          # ldo > N: a gap behind every row
    for q in c["groups"]:
        k, nb = q["k"], q["nb"]
        KB = k // 32
        wp = ops.pack_gate_up(q["w"][0].to(dev), q["w"][1].to(dev)) if epi == SWIGLU else ops.pack_weight(q["w"][0].to(dev))
        pk = w12.pack(wp.view(torch.int16), KB)
        assert pk is not None, "not packable: a block over the exception cap"
        data, meta = pk
        assert data.numel() == nb * KB * 768 and meta.numel() == nb * w12.META
        assert torch.equal(w12.unpack(data, meta, KB), wp.view(torch.int16))
        if q.get("planted"):
            cnt = w12.exceptions_per_block(meta)
            assert int(cnt.min()) >= 16 and int(cnt.max()) <= 32
            if q.get("full"):
                assert int(cnt[0]) == 32          # one block with exactly 32 exceptions: the list ends at the sentinel in word 32
        wpad = torch.full((data.numel() + 3 * KB * 768,), 0xFF, dtype=torch.uint8, device=dev)      # 0xFF behind n_blocks
        wpad[:data.numel()] = data
        mpad = torch.cat([meta.to(dev), nan_records(3, KB, dev)])                                   # NaN-patching records behind n_blocks
        src = torch.full((tiles * 16 + 2, k + 8), NAN, dtype=bf16, device=dev)                      # NaN pad rows (and columns behind K) in the source
        src[:rows, :k] = q["A"].to(dev)
        b = torch.full((tiles * 16 * k + 64,), SENT, dtype=bf16, device=dev)
        ops.pack_rows(src[:rows, :k], out=b)
        q["packed"] = b
        if epi == SWIGLU:
            o = torch.full((tiles * 16 * q["N"] + 64,), SENT, dtype=bf16, device=dev)
        else:
            o = torch.full((tiles * 16 + 4, ldo), SENT, dtype=bf16, device=dev)
        ws.append(wpad); ms.append(mpad); bs.append(b); outs.append(o)
    if call is None:
        ops.gemm_wide_w12(ws, ms, [q["nb"] for q in c["groups"]], [q["k"] for q in c["groups"]], rows, bs, outs, epilogue=epi, waves=c["waves"],
                          u=c["u"], n_valid=None if epi == SWIGLU else c["n_valid"])
    else:
        call(ws, ms, bs, outs)
    torch.cuda.synchronize()
    return [o.cpu() for o in outs]


# (launch, K per group, n_blocks per group): 3, 1 and 11 groups
KERNEL_CASES = [("gate_up", [2048, 2048, 2048], [12, 4, 20]), ("gate_up", [512], [12]), ("down", [2752, 2752, 2752], [3, 5, 1]),
                ("down", [1376, 1376, 1376], [3, 5, 1]), ("down", [2752, 1376, 2752], [3, 5, 1]), ("down", [1376], [5]),
                ("gate_up", [2048] * 11, [4, 8, 4, 12, 4, 4, 8, 4, 4, 4, 8]), ("down", [2752, 1376] * 5 + [2752], [1, 2, 3, 1, 2, 1, 1, 3, 1, 2, 1])]


def compare_with_the_bf16_kernel(dev, rows, planted):
    for n, (name, ks, nbs) in enumerate(KERNEL_CASES):
        c = gauss12(name, rows, ks, nbs, 100 * rows + n + (50 if planted else 0), planted=planted)
        want = run_wide(c, dev)
        check_guards(c, want)
        got = run_wide_w12(c, dev)
        check_guards(c, got)
        for q, o, w in zip(c["groups"], got, want):          # the whole buffers: results, pad rows, gaps and margins
            assert torch.equal(bits(o), bits(w)), (name, rows, ks, q["k"], int((bits(o) != bits(w)).sum()))


@pytest.mark.parametrize("rows", ROWS)
def test_w12_wide_bit_for_bit_against_the_bf16_wide_kernel_on_the_same_weights(dev, rows):
    compare_with_the_bf16_kernel(dev, rows, False)


@pytest.mark.parametrize("rows", ROWS)
def test_w12_wide_with_planted_exceptions_bit_for_bit(dev, rows):
    compare_with_the_bf16_kernel(dev, rows, True)


def test_planted_exceptions_sit_where_the_cursor_turns():
    """the plan of plant() itself: in every block an entry at the first and at the last k-step of every wave's slice, for both U and the
    uneven split, in all four K quarters, both k-steps of a chunk, and two entries in one k-step of one block"""
    from unimoe_audio_amd import w12
    for K, U in ((2048, 1), (512, 1), (2752, 2), (1376, 2)):
        KB = K // 32
        W = plant((torch.randn(48, K, generator=torch.Generator().manual_seed(K)) * 0.02).to(bf16), U, blk32=0)
        pk = w12.pack(w12.wp16_from_rows(W).view(torch.int16), KB)
        assert pk is not None
        m = pk[1].view(3, w12.META).to(torch.int64) & 0xFFFFFFFF
        cnt = w12.exceptions_per_block(pk[1]).tolist()
        assert cnt[0] == 32 and 18 <= cnt[1] <= 18 + 9 and 16 <= cnt[2] <= 16 + 9, (K, cnt)          # (planted + at most 9 natural ones)
        if KB == 43:
            assert [a for a, _ in wide_wave_steps(KB, U, WV)] == [0, 5, 10, 16, 21, 26, 32, 37]
        for nb in range(3):
            ent = m[nb, :cnt[nb]]
            steps, lanes = (ent >> 25).tolist(), ((ent >> 19) & 63).tolist()
            for i0, i1 in wide_wave_steps(KB, U, WV):
                assert i0 in steps and i1 - 1 in steps, (K, nb, i0, i1)
            assert {l >> 4 for l in lanes} == {0, 1, 2, 3}
            assert {s & 1 for s in steps} == {0, 1}
        s1 = (m[1, :cnt[1]] >> 25).tolist()
        assert max(s1.count(s) for s in set(s1)) >= 2


@pytest.mark.parametrize("rows", [34, 64])
def test_w12_wide_exact_against_fp64(dev, rows):
    """the small-integer data of test_gpu_wide_gemm with the zero weights replaced by 1 / 16 (a zero is an exception; a ninth of a matrix
    is over the cap): weights k / 16 with 1 <= |k| <= 4, every product and sum exact in fp32"""
    for name, K, n_groups in [("gate_up", 2048, 1), ("down", 2752, 3), ("down", 1376, 3)]:
        c = make(name, rows, K, n_groups, "int", 3000 * rows + K)
        for q in c["groups"]:
            q["w"] = [torch.where(w == 0, torch.full_like(w, 1 / 16), w) for w in q["w"]]
        outs = run_wide_w12(c, dev)
        check_guards(c, outs)
        check_fp64(c, outs)


def test_w12_wide_refusals(dev):
    from unimoe_audio_amd import _lib, ops
    down = gauss12("down", 64, [1376], [4], 1)                # (buffers of 64 rows: every row count below fits them)
    gate = gauss12("gate_up", 64, [2048], [4], 2)
    # (case, rows, epilogue, waves, u, n_blocks, K, how the pointers are bent, what the message names)
    cases = [(down, 16, BF16, 8, 2, 4, 1376, None, "rows"), (down, 65, BF16, 8, 2, 4, 1376, None, "rows"),
             (down, 32, BF16, 8, 1, 4, 1376, None, "epilogue, waves, u"), (down, 32, F32, 8, 2, 4, 1376, None, "epilogue, waves, u"),
             (down, 32, SWIGLU, 4, 1, 4, 1376, None, "epilogue, waves, u"), (down, 32, RESID, 4, 16, 4, 1376, None, "epilogue, waves, u"),
             (down, 32, BF16, 8, 2, 4, 1360, None, "host_k"),                 # K % 32 != 0
             (down, 32, BF16, 8, 2, 4, 127 * 32, None, "host_k"),             # KB >= 127
             (down, 32, BF16, 8, 2, 4, 1376, "no_w", "host_w12"), (down, 32, BF16, 8, 2, 4, 1376, "no_meta", "host_meta"),
             (down, 32, BF16, 8, 2, 4, 1376, "w+8", "host_w12"), (down, 32, BF16, 8, 2, 4, 1376, "meta+2", "host_meta"),
             (gate, 32, SWIGLU, 8, 1, 3, 2048, None, "host_n_blocks"),        # 3 blocks: no gate/up fours
             (gate, 32, SWIGLU, 8, 1, 4, 2304, None, "host_k"),               # K % 512 != 0: a wave slice would not be whole chunks
             (gate, 32, SWIGLU, 8, 1, 4, 1376, None, "host_k")]
    for c, rows, epi, waves, u, nb, k, bend, names in cases:
        def call(ws, ms, bs, outs):
            if bend == "no_w":
                ws = [None]
            elif bend == "no_meta":
                ms = [None]
            elif bend == "w+8":
                ws = [ws[0][8:]]
            elif bend == "meta+2":
                ms = [ms[0].view(torch.uint8)[2:]]
            with pytest.raises(_lib.UmoeError) as err:
                ops.gemm_wide_w12(ws, ms, [nb], [k], rows, bs, outs, epilogue=epi, waves=waves, u=u, n_valid=None if epi == SWIGLU else 16 * nb)
            assert "umoe_gemm_wide_w12" in str(err.value) and names in str(err.value), (names, str(err.value))
        for o in run_wide_w12(c, dev, call):
            assert bool((o == SENT).all()), (rows, epi, waves, u, nb, k, bend)          # nothing was launched


# ------------------------------------------------------------------------------------------------ engine
def experts(m, layers=None):
    for li, layer in enumerate(m.language_model.layers):
        if layers is None or li in layers:
            for e in list(layer.mlp.dynamic_real_moe.deepspeed_moe.experts.deepspeed_experts) + list(layer.mlp.fixed_real_moe):
                yield e


@pytest.fixture(scope="module")
def worlds(dev):
    """the two-layer full-width model of test_gpu_wide_decode and the prompt pairs of 32 requests, in three kinds: as built; with
    exceptions planted in every block of every expert matrix (test_gpu_w12.plant); with a block of the LAST layer over the cap"""
    from test_gpu_engine import prompt
    from test_gpu_fp8 import build, ref_cfg
    from test_gpu_w12 import plant as plant_flat
    cfg = ref_cfg()
    ids, am, codec = prompt(cfg, 32, T, 6, [3, 0, 1, 0, 2, 0, 0, 4] + [0] * 40 + [1, 2, 0, 5] + [0] * 12)
    made = {}

    def world(kind):
        if kind not in made:
            m = build(cfg, 41)
            if kind == "planted":
                for e in experts(m):
                    for lin in (e.gate_proj, e.up_proj, e.down_proj):
                        plant_flat(lin.weight.data)
            elif kind == "overcap":
                with torch.no_grad():          # 48 exceptions in block 1 of a shared expert's down weights of the last layer
                    m.language_model.layers[1].mlp.fixed_real_moe[0].down_proj.weight[16:32, :3] = 0
            m = m.to(dev)
            with torch.no_grad():
                x = m.calculate_input_embedding(ids.to(dev), codec.to(dev)).reshape(64, T, cfg.hidden_size).contiguous()
            made[kind] = dict(m=m, cfg=cfg, x=x, am=am, dev=dev, cache={})
        return made[kind]

    yield world
    for w in made.values():
        if w["m"]._engine is not None:
            w["m"]._engine.close()


def run12(world, monkeypatch, w12_wide, reqs, steps, settings, graph, env=None):
    """test_gpu_wide_decode.run with DecodeEngine(..., w12_wide=w12_wide), plus the logits of the last step and expert_w12"""
    import unimoe_audio_amd.model as M
    key = (w12_wide, tuple(reqs), steps, settings["do_sample"], graph, env)
    if key in world["cache"]:
        return world["cache"][key]
    real = M.DecodeEngine

    def engine(m, B, **kw):
        return real(m, B, w12_wide=w12_wide, **kw)

    with monkeypatch.context() as mp:
        mp.setattr(M, "DecodeEngine", engine)
        mp.setenv("UMOE_WIDE_DECODE", "1")
        if env is not None:
            mp.setenv("UMOE_WIDE_W12", env)
        out, eng = run(dict(world, cache={}), reqs, steps, settings, graph, keep_engine=True)
    cfg = world["cfg"]
    out["logits"] = eng.copy_buffer("logits", torch.float32, (2 * len(reqs), cfg.codec_channels * cfg.codec_vocab_size)).cpu()
    out["w12"] = eng.info("expert_w12")
    eng.close()
    world["cache"][key] = out
    return out


def same_engine_output(a, b, what):
    for k in ("k", "v", "tokens", "state", "mask", "topk", "logits"):
        assert torch.equal(a[k], b[k]), (what, k)
    assert a["lengths"] == b["lengths"], what


def on_against_off(world, monkeypatch, B, graph, want_w12=1):
    reqs = list(range(B))
    on = run12(world, monkeypatch, True, reqs, 6, SAMPLED, graph)
    off = run12(world, monkeypatch, False, reqs, 6, SAMPLED, graph)
    assert on["launch"] == 4 and on["w12"] == want_w12 and on["tiles"] == (2 * B + 15) // 16 and on["tiles"] in (2, 3, 4) and on["handoff"] == 0
    assert off["launch"] == 4 and off["w12"] == 0 and off["tiles"] == on["tiles"]
    same_engine_output(on, off, f"B={B}")
    assert len({tuple(on["tokens"][b].flatten().tolist()) for b in range(B)}) > B // 4          # (the requests do differ)
    return on


@pytest.mark.parametrize("B,graph", [(16, False), (16, True), (24, False), (32, False), (9, False)], ids=["16-eager", "16-graph", "24", "32", "9"])
def test_w12_wide_engine_equals_the_engine_without_the_switch(worlds, monkeypatch, B, graph):
    on_against_off(worlds("plain"), monkeypatch, B, graph)


@pytest.mark.parametrize("B,graph", [(16, True), (24, False), (9, False)], ids=["16-graph", "24", "9"])
def test_w12_wide_engine_with_planted_exceptions_in_every_expert_matrix(worlds, monkeypatch, B, graph):
    from unimoe_audio_amd import w12
    world = worlds("planted")
    pk = world["m"].packed_w12()
    assert all(l is not None for l in pk)
    for l in pk:                           # every block of every matrix carries its 16 planted exceptions
        for d, meta in l["gu"] + l["dn"]:
            assert int(w12.exceptions_per_block(meta).min()) >= 16
    on_against_off(world, monkeypatch, B, graph)


def test_last_layer_over_the_cap_runs_the_wp16_launches(worlds, monkeypatch):
    world = worlds("overcap")
    pk = world["m"].packed_w12()
    assert pk[0] is not None and pk[1] is None
    on_against_off(world, monkeypatch, 16, False, want_w12=0)      # ("expert_w12" speaks of the last layer: it ran the WP16 launches)


def test_wide_w12_env_forces_the_wp16_launches(worlds, monkeypatch):
    world = worlds("plain")
    reqs = list(range(16))
    forced = run12(world, monkeypatch, True, reqs, 6, SAMPLED, False, env="0")
    assert forced["launch"] == 4 and forced["w12"] == 0 and forced["tiles"] == 2
    on = run12(world, monkeypatch, True, reqs, 6, SAMPLED, False)
    assert on["w12"] == 1
    same_engine_output(forced, on, "UMOE_WIDE_W12=0")
    # 8 requests: the switch does not reach the flat launch (it streams WP12 on its own account, as before)
    small = run12(world, monkeypatch, True, list(range(8)), 6, SAMPLED, False)
    plain = run12(world, monkeypatch, False, list(range(8)), 6, SAMPLED, False)
    assert small["launch"] == plain["launch"] == 2 and small["w12"] == plain["w12"] == 1 and small["tiles"] == 1
    same_engine_output(small, plain, "8 requests")


def test_w12_wide_serving_of_12_rows_equals_bf16_serving(worlds, monkeypatch):
    """a few admissions at different steps, row 10 used twice, one step graph captured and replayed across them: the engine model.engine()
    builds with w12_wide=True against the one it builds with w12_wide=False"""
    monkeypatch.setenv("UMOE_WIDE_DECODE", "1")              # (12 rows: not the bf16 engine's default)
    world = worlds("plain")
    m = world["m"]
    plan = {0: [(r, r) for r in range(5)], 3: [(ROW, 20), (7, 9)], 20: [(11, 21)], 40: [(8, 23)], 60: [(ROW, 22)]}
    monkeypatch.setattr(m, "engine", functools.partial(type(m).engine, m, w12_wide=True))
    got, c12 = serve_run(world, plan, True)
    assert m._engine.expert_weights == "bf16" and m._engine.w12_wide and m._engine.info("expert_w12") == 1
    m._engine.close()
    m._engine = None
    monkeypatch.setattr(m, "engine", functools.partial(type(m).engine, m, w12_wide=False))
    ref, c16 = serve_run(world, plan, True)
    assert not m._engine.w12_wide and m._engine.info("expert_w12") == 0
    m._engine.close()
    m._engine = None
    assert c12 == c16 == 1                                   # one graph capture across the admissions
    assert sorted(got) == sorted(ref) == [0, 1, 2, 3, 4, 9, 20, 21, 22, 23]
    for b in got:
        assert got[b][1] == ref[b][1] and torch.equal(got[b][0], ref[b][0]) and got[b][2] == ref[b][2], b
