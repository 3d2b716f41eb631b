"""A few eager decode steps of the full 36-layer model at one batch size, to be run under a counter-only profiler pass:

    rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR -o f -- python scripts/wide_pmc_step.py --batch 16 --steps 5

UMOE_WIDE_DECODE selects the leg.  scripts/summarize_wide_pmc.py turns the passes of both legs into profiles/wide_decode_pmc.md."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--prompt", type=int, default=300)
    a = ap.parse_args()
    from unimoe_audio_amd.codec_utils import prepare_audio_prompt
    from unimoe_audio_amd.model import DecodeEngine
    args = argparse.Namespace(layers=0, codec_channels=0)
    dev = torch.device("cuda:0")
    cfg = bench.make_cfg(args)
    model, _ = bench.build_model(cfg, dev)
    B, T = a.batch, a.prompt
    eng = DecodeEngine(model, B, Lmax=T + 136, Tmax=128)
    ids, am, codec = bench.synth_prompt(cfg, B, T, dev)
    eng.prefill(model.calculate_input_embedding(ids, codec).reshape(-1, cfg.hidden_size).contiguous(), am)
    pre, psteps = prepare_audio_prompt(cfg, [None] * B)
    eng.start_decode(pre, psteps, 64, 64, cfg_scale=3.0, temperature=1.2, top_p=0.95, top_k=45, eos_mul=0.8, do_sample=True, seed=1234)
    for _ in range(a.steps):
        eng.step(False)
    torch.cuda.synchronize()
    E = cfg.num_experts
    masks = eng.copy_buffer("all_mask", torch.int32, (cfg.num_hidden_layers, 2 * B, E)).cpu()
    hit = (masks[:, :, : cfg.mlp_dynamic_expert_num].sum(1) > 0).sum(1).float().mean()
    print(f"expert_launch {eng.info('expert_launch')} row_tiles {eng.info('row_tiles')} mean_experts_hit {float(hit):.3f} kv_len {T + a.steps}")
    eng.close()


if __name__ == "__main__":
    main()
