"""The decode engine's attention at long context, layer by layer against the CPU oracle (the probe pattern of
test_gpu_fulldepth.py::test_full_depth_every_layer_in_isolation_vs_oracle) on the reference's attention geometry: hidden 2048,
16 / 2 heads (GQA group 8), two layers with small experts so the oracle stays cheap.

A ~1000-token prompt with different left pads per row: at 8 key splits every wave of every split holds at least two 16-key tiles,
so the double-buffered tile loop, the 4-wave merge and the 8-way combine all run with real work in every part (the other engine
tests stay at <= 112 keys, where only wave 0 of the first splits sees a key).  Repeated at 1 and 3 splits (direct write, generic
combine).  Each layer reads the ORACLE's residual input and KV cache, so the attention half (x1 - x_in) is compared per layer at the
full-depth test's criteria; the same step through graph replay must give logits bit-identical to eager launches."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# the full-depth test's bounds (test_gpu_fulldepth.PER_LAYER_BOUNDS, attn_half) and its fp32-centre criterion
ATTN_HALF = 0.003


@pytest.fixture(scope="module")
def long_case():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from oracle import decode as OD
    from test_gpu_engine import build, prompt, small_cfg
    dev = torch.device("cuda:0")
    cfg = small_cfg(hidden_size=2048, num_attention_heads=16, num_key_value_heads=2)
    assert cfg.head_dim == 128 and cfg.num_hidden_layers == 2
    m, w = build(cfg, 11, 0.02)
    B, T, MAXT = 1, 1020, 48
    # cached keys at the first decode step: 1020 and 1012 -> chunk 128 at 8 splits, the last split 124 / 116 keys (>= 113: every
    # wave of every split has two tiles)
    pads = [0, 8]
    ids, am, codec = prompt(cfg, B, T, 12, pads)
    rows = 2 * B
    pre, psteps = OD.prepare_audio_prompt(cfg, [None] * B)
    step0 = min(psteps) - 1
    g = torch.Generator().manual_seed(13)
    forced = torch.randint(0, 1024, (B, max(pre.shape[1], step0 + 3), cfg.codec_channels), generator=g).to(torch.int32)
    keep = pre.to(torch.int32) != -1
    forced[:, : pre.shape[1]][keep] = pre.to(torch.int32)[keep]
    tm = OD.TextModelOracle(cfg, w)
    key_valid = am.bool()
    pos = (am.long().cumsum(-1) - 1).masked_fill(am == 0, 1)
    x = OD.input_embedding(cfg, w, ids, codec)
    kv1 = torch.cat([key_valid, torch.ones((rows, 1), dtype=torch.bool)], -1)
    p1 = (kv1.long().cumsum(-1) - 1).masked_fill(~kv1, 1)[:, -1:]
    tok2 = forced[:, step0: step0 + 1].long().repeat_interleave(2, dim=0)
    with torch.no_grad():
        _, cache, _ = tm.forward(x, key_valid, pos, None)
        _, _, lay = tm.forward(OD.codec_embedding(cfg, w, tok2), kv1, p1, cache, collect_router=True)
    x_in = torch.stack([r["x_in"][:, 0] for r in lay])
    x1_o = torch.stack([r["x1"][:, 0] for r in lay]).float()
    # fp32 centre on the same inputs (the bf16 oracle's layer inputs and KV cache, upcast)
    w32 = {k: v.float() for k, v in w.items()}
    with torch.no_grad():
        c32 = [(k.float(), v.float()) for k, v in cache]
        _, _, lay32 = OD.TextModelOracle(cfg, w32).forward(OD.codec_embedding(cfg, w32, tok2), kv1, p1, c32, collect_router=True,
                                                            layer_inputs=[t[:, None].float() for t in x_in])
    x1_c = torch.stack([r["x1"][:, 0] for r in lay32])
    del w32, c32, lay32
    gm = m.to(dev)
    xg = gm.calculate_input_embedding(ids.to(dev), codec.to(dev))
    assert torch.equal(xg.cpu(), x)
    yield dict(cfg=cfg, gm=gm, dev=dev, B=B, T=T, MAXT=MAXT, am=am, xg=xg, forced=forced, psteps=psteps, cache=cache, x_in=x_in,
               x1_o=x1_o, x1_c=x1_c, rows=rows)
    del gm
    torch.cuda.empty_cache()


def _engine(c, splits):
    from unimoe_audio_amd.model import DecodeEngine
    cfg = c["cfg"]
    eng = DecodeEngine(c["gm"], c["B"], Lmax=c["T"] + c["MAXT"] + 8, Tmax=c["MAXT"] + 64, attn_splits=splits)
    eng.prefill(c["xg"].reshape(-1, cfg.hidden_size).contiguous(), c["am"].to(c["dev"]))
    return eng


def _start(c, eng):
    eng.start_decode(c["forced"], c["psteps"], c["MAXT"], 6, cfg_scale=3.0, temperature=1.0, top_p=1.0, top_k=45, eos_mul=0.8,
                     do_sample=False)


@pytest.mark.parametrize("splits", [8, 1, 3])
def test_attention_half_per_layer_at_1000_keys_vs_oracle(long_case, splits):
    c = long_case
    cfg, dev, T, rows = c["cfg"], c["dev"], c["T"], c["rows"]
    Lyr, KVH, hd = cfg.num_hidden_layers, cfg.num_key_value_heads, cfg.head_dim
    eng = _engine(c, splits)
    Lmax = eng.Lmax
    for name, idx in (("k_cache", 0), ("v_cache", 1)):
        full = torch.zeros(Lyr, rows, KVH, Lmax, hd, dtype=torch.bfloat16)
        full[:, :, :, :T] = torch.stack([kv[idx] for kv in c["cache"]])
        eng.write_buffer(name, full.to(dev))
    _start(c, eng)
    pr = eng.set_probe(teach_x=c["x_in"].to(dev), dump_x1=True)
    eng.step(use_graph=False)
    torch.cuda.synchronize()
    assert eng.handoff_error() == 0
    x1_h = pr["x1"].cpu().float()
    eng.set_probe()
    eng.close()
    xin, x1_o, x1_c = c["x_in"].float(), c["x1_o"], c["x1_c"]
    fro = lambda t: float(t.norm())
    att = [fro(x1_h[l] - x1_o[l]) / fro(x1_o[l] - xin[l]) for l in range(Lyr)]
    vs_c_hip = [fro(x1_h[l] - x1_c[l]) / fro(x1_c[l] - xin[l]) for l in range(Lyr)]
    vs_c_orc = [fro(x1_o[l] - x1_c[l]) / fro(x1_c[l] - xin[l]) for l in range(Lyr)]
    print(f"\nLONG-CONTEXT ATTENTION splits={splits}: attn_half_rel {att} vs fp32: hip {vs_c_hip} oracle {vs_c_orc}")
    assert max(att) < ATTN_HALF, att
    # no further from the fp32 walk than the CPU oracle (x 1.25 + 0.002, averaged over the layers)
    assert sum(vs_c_hip) / Lyr < 1.25 * sum(vs_c_orc) / Lyr + 0.002, (vs_c_hip, vs_c_orc)


@pytest.mark.parametrize("splits", [8, 1, 3])
def test_graph_replay_equals_eager_at_1000_keys(long_case, splits):
    c = long_case
    cfg = c["cfg"]
    got = {}
    for use_graph in (False, True):
        eng = _engine(c, splits)
        _start(c, eng)
        eng.step(use_graph=use_graph)
        got[use_graph] = eng.copy_buffer("logits", torch.float32, (c["rows"], cfg.codec_channels * cfg.codec_vocab_size)).cpu()
        eng.close()
    assert torch.equal(got[True], got[False])
    assert bool(torch.isfinite(got[False]).all())
