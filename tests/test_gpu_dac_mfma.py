"""The DAC convolutions on the f32 MFMA (csrc/umoe_dac_mfma.hip, conv_form="mfma" of dac.py) on the GPU.

The kernels tile 64 output channels x 64 output positions per workgroup (one tile height, one tile width) and walk the reduction
(input channel, tap) in k-chunks of 32; the transposed form tiles 64 positions PER PHASE.  Launchers of this file call the six _mfma
entries directly; cases, float64 references, bounds and checkers are those of tests/test_gpu_dac_fp64.py (its bound
(n + 2) u S + u |ref| holds for any summation order, so it covers the MFMA's fmaf chain unchanged).

  vs float64    every case of that file's CONV_GROUPS / CONVT_GROUPS, each with and without Snake.  For conv1d its Cout 1 / 63 / 64 / 65 /
                130 and Lout 1 / 63 / 64 / 65 / 129 are the edges of this kernel's 64 x 64 tile too.  For the transposed form they are
                not: its position tile is 64 values of q = (t + pad) / stride per phase, and that file's cases have L <= 33 (one q tile)
                and Cout 1 / 5 / 65.  So EDGE adds transposed cases whose q count (L + 1 at K = 2 stride, pad = stride / 2) is 63 / 64 /
                65 / 66 / 129 / 130 at stride 2 and 65 / 129 at stride 4 -- one, two and three q tiles, the first q of a phase before
                the first output, the last past the last -- and Cout 63 / 64 / 65 / 130; and for both forms the reduction length Cin K
                (Cin M) at 1, 7, 9, 31, 32, 33 and 65.  WIDE: the product's widest layers once at short length (1536 -> 768 transposed
                K 16 stride 8 at L = 4; 768 -> 768 K 7 dilation 9 with the residual at L = 64).  GUARD sentinels around every output.
  exact         small-integer data (|x|, |w|, |bias| <= 4, no Snake): bit for bit the float64 convolution, no tolerance.
  windows       that file's windows, on its cases and on EDGE (so windows [1, Lout - 1) that span two and three q tiles of the transposed
                form, and rows of one launch with one and with three q tiles), through _win_mfma (against float64, NaN in the MARGIN,
                sentinel outside) and through _win_rows_mfma with 3 rows -- two batch planes on different windows, the middle row idle;
                every stored output bit-identical to the same position of the full _mfma launch.
  refusals      every bad argument, empty output, window and table fault the direct siblings refuse, and what these kernels cannot
                launch; through the C entries and dac.conv1d(form="mfma"); nothing written.  (The direct kernels' LDS refusal has no
                counterpart: LDS use is fixed, and that geometry -- K 32 at stride 8 -- is computed here and checked against float64.)
  model         a small random DacModel in "mfma": encode / decode against the fp32 torch walk of tests/test_gpu_dac.py, both streaming
                decoders bit-identical to DacModel.decode, serve(stream=True) == serve(stream=False) in wav bytes, and "direct" still
                gives the bytes it gave before set_conv_form.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import test_gpu_dac_fp64 as F64
from test_gpu_dac_fp64 import (B, CONV_GROUPS, CONVT_GROUPS, GUARD, SENT, Stats, _p, _stream, c1, check_conv, check_win, conv_case, ct,
                               keeps_sentinel, last_error, win_buffers, windows_of)

pytestmark = pytest.mark.gpu
f64 = torch.float64

EDGE = {
    "conv": [c1("m_r1", 1, 5, 1, 70), c1("m_r7", 1, 5, 7, 70, pad=3), c1("m_r9", 3, 5, 3, 70, pad=1), c1("m_r31", 31, 5, 1, 70),
             c1("m_r32", 32, 5, 1, 70), c1("m_r33", 11, 5, 3, 70, pad=1), c1("m_r65", 13, 66, 5, 130, dil=2, pad=4, resid=True),
             c1("m_lds", 8, 8, 32, 600, stride=8, pad=4)],
    "convt": [ct("m_t_r1", 1, 5, 4, 20, 4, 1), ct("m_t_r7", 7, 5, 4, 20, 4, 1), ct("m_t_r9", 9, 5, 5, 20, 5, 1), ct("m_t_r31", 31, 5, 4, 20, 4, 1),
              ct("m_t_r32", 16, 5, 8, 20, 4, 2), ct("m_t_r33", 11, 5, 9, 20, 4, 2), ct("m_t_r34", 17, 65, 16, 20, 8, 4)] +
             # the q tile of 64 per phase: q runs over L + 1 values (K = 2 stride, pad = stride / 2), and the channel tile's edges
             [ct(f"m_t_q{L + 1}_co{co}", 9, co, 4, L, 2, 1) for L, co in ((62, 63), (63, 64), (64, 65), (65, 5), (128, 64), (129, 130))] +
             [ct(f"m_t_s4_q{L + 1}_co{co}", 9, co, 8, L, 4, 2) for L, co in ((64, 63), (128, 5))],
}
WIDE = [dict(ct("m_wide_t", 1536, 768, 16, 4, 8, 4), snakes=(True,)),
        dict(c1("m_wide_c", 768, 768, 7, 64, dil=9, pad=27, resid=True), snakes=(True,))]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    from unimoe_audio_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def lib():
    from unimoe_audio_amd import _lib as L
    return L.lib()


def case_of(spec, snake):
    """conv_case of a spec of this file (that function looks its spec up by name)"""
    F64.SPECS[spec["name"]] = spec
    try:
        return conv_case(spec["name"], snake)
    finally:
        del F64.SPECS[spec["name"]]


def on_dev(c, dev):
    from unimoe_audio_amd import dac as D
    d = F64.on_dev(c, dev)
    if "wt" not in d:
        d["wt"] = D.kmajor(c["w"], c["kind"] == "convt").to(dev)
        assert tuple(d["wt"].shape) == (c["Cin"], c["K"], c["Cout"]) and d["wt"].is_contiguous()
    return d


def launch_full(c, dev):
    """the full-sequence _mfma kernel into the middle of a sentinel buffer -> y [B][Cout][Lout] (on the device); the guards are checked"""
    d = on_dev(c, dev)
    nb = c["x"].shape[0]
    numel = nb * c["Cout"] * c["Lout"]
    buf = torch.full((numel + 2 * GUARD,), SENT, dtype=torch.float32, device=dev)
    y = C.c_void_p(buf.data_ptr() + 4 * GUARD)
    lo = C.c_int(-1)
    if c["kind"] == "conv":
        rc = lib().umoe_dac_conv1d_mfma(_p(d["x"]), _p(d["wt"]), _p(d["b"]), _p(d["alpha"]), _p(d["resid"]), nb, c["Cin"], c["L"], c["Cout"], c["K"],
                                        c["stride"], c["dil"], c["pad"], int(c["tanh"]), y, C.byref(lo), _stream())
    else:
        rc = lib().umoe_dac_conv_transpose1d_mfma(_p(d["x"]), _p(d["wt"]), _p(d["b"]), _p(d["alpha"]), nb, c["Cin"], c["L"], c["Cout"], c["K"],
                                                  c["stride"], c["pad"], c["out_pad"], y, C.byref(lo), _stream())
    assert rc == 0, (c["name"], last_error())
    assert lo.value == c["Lout"], (c["name"], lo.value, c["Lout"])
    keeps_sentinel(f"{c['name']}: before y", buf[:GUARD].cpu())
    keeps_sentinel(f"{c['name']}: behind y", buf[GUARD + numel:].cpu())
    return buf[GUARD:GUARD + numel].view(nb, c["Cout"], c["Lout"])


def launch_win(c, wb, dev):
    d = on_dev(c, dev)
    x, r, y = wb["x"].to(dev), (None if wb["r"] is None else wb["r"].to(dev)), wb["y"].to(dev)
    if c["kind"] == "conv":
        rc = lib().umoe_dac_conv1d_win_mfma(_p(x), wb["x_off"], x.shape[2], _p(d["wt"]), _p(d["b"]), _p(d["alpha"]), _p(r), wb["r_off"],
                                            0 if r is None else r.shape[2], B, c["Cin"], c["L"], c["Cout"], c["K"], c["stride"], c["dil"], c["pad"],
                                            int(c["tanh"]), wb["t0"], wb["n"], _p(y), wb["y_off"], y.shape[2], _stream())
    else:
        rc = lib().umoe_dac_conv_transpose1d_win_mfma(_p(x), wb["x_off"], x.shape[2], _p(d["wt"]), _p(d["b"]), _p(d["alpha"]), B, c["Cin"], c["L"],
                                                      c["Cout"], c["K"], c["stride"], c["pad"], c["out_pad"], wb["t0"], wb["n"], _p(y), wb["y_off"],
                                                      y.shape[2], _stream())
    assert rc == 0, (c["name"], wb["t0"], wb["n"], last_error())
    return y


def launch_rows(c, picks, dev):
    """picks: per row None (idle) or (batch plane, window buffers); one _win_rows_mfma launch -> the rows' y planes [Cout][Ly] (None: idle)"""
    from unimoe_audio_amd.dac import dac_row_words
    d = on_dev(c, dev)
    keep, words, ys = [], [], []
    for pick in picks:
        if pick is None:
            words.append(dac_row_words())
            ys.append(None)
            continue
        b, wb = pick
        x = wb["x"][b].to(dev).contiguous()
        r = None if wb["r"] is None else wb["r"][b].to(dev).contiguous()
        y = wb["y"][b].to(dev).contiguous()
        keep += [x, r]
        ys.append(y)
        words.append(dac_row_words(x=x.data_ptr(), resid=0 if r is None else r.data_ptr(), y=y.data_ptr(), x_off=wb["x_off"], Lx=x.shape[1],
                                   r_off=wb["r_off"], Lr=0 if r is None else r.shape[1], y_off=wb["y_off"], Ly=y.shape[1], t_begin=wb["t0"], n=wb["n"],
                                   L=c["L"]))
    host = torch.tensor(words, dtype=torch.int64)
    table = host.to(dev)
    max_n = max(w[10] for w in words)
    if c["kind"] == "conv":
        rc = lib().umoe_dac_conv1d_win_rows_mfma(_p(host), _p(table), len(picks), max_n, _p(d["wt"]), _p(d["b"]), _p(d["alpha"]), c["Cin"], c["Cout"],
                                                 c["K"], c["stride"], c["dil"], c["pad"], int(c["tanh"]), _stream())
    else:
        rc = lib().umoe_dac_conv_transpose1d_win_rows_mfma(_p(host), _p(table), len(picks), max_n, _p(d["wt"]), _p(d["b"]), _p(d["alpha"]), c["Cin"],
                                                           c["Cout"], c["K"], c["stride"], c["pad"], c["out_pad"], _stream())
    assert rc == 0, (c["name"], last_error())
    torch.cuda.synchronize()
    return ys


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def cases_of(specs):
    return [case_of(s, sn) for s in specs for sn in s["snakes"]]


# ================================================================================================ per element against float64
@pytest.mark.parametrize("group", list(CONV_GROUPS) + list(CONVT_GROUPS))
def test_fp64_file_cases_vs_fp64(dev, group):
    st = Stats()
    for s in (CONV_GROUPS.get(group) or CONVT_GROUPS[group]):
        for sn in s["snakes"]:
            c = conv_case(s["name"], sn)
            check_conv(c, launch_full(c, dev), st, s["name"] + ("+snake" if sn else ""))
    st.show(f"mfma {group}")


@pytest.mark.parametrize("kind", ["conv", "convt"])
def test_reduction_edges_vs_fp64(dev, kind):
    """Cin K (Cin M) around the MFMA k-step of 4 and the k-chunk of 32: the zero-filled tail steps"""
    st = Stats()
    for c in cases_of(EDGE[kind]):
        check_conv(c, launch_full(c, dev), st, c["name"] + ("+snake" if c["snake"] else ""))
    st.show(f"mfma reduction edges {kind}")


@pytest.mark.parametrize("i", [0, 1], ids=["convt_1536_768", "conv_768_768_d9"])
def test_widest_layers_vs_fp64(dev, i):
    st = Stats()
    c = case_of(WIDE[i], True)
    check_conv(c, launch_full(c, dev), st)
    st.show("mfma widest layer")


def _int_case(kind, Cin, Cout, K, L, stride, dil, pad, out_pad, seed):
    g = torch.Generator().manual_seed(seed)
    ri = lambda *shape: torch.randint(-4, 5, shape, generator=g).float()      # noqa: E731
    c = dict(kind=kind, name=f"int_{kind}_{Cin}_{Cout}_{K}_{stride}", Cin=Cin, Cout=Cout, K=K, L=L, stride=stride, dil=dil, pad=pad, out_pad=out_pad,
             tanh=False, x=ri(B, Cin, L), w=ri(*((Cout, Cin, K) if kind == "conv" else (Cin, Cout, K))), b=ri(Cout), alpha=None)
    c["Lout"] = F64.out_len(c)
    c["resid"] = ri(B, Cout, c["Lout"]) if kind == "conv" else None
    ref = F64._conv(c, c["x"].to(f64), c["w"].to(f64), c["b"].to(f64))
    c["ref"] = ref if c["resid"] is None else ref + c["resid"].to(f64)
    assert float(c["ref"].abs().max()) < 2 ** 24 and Cin * K * 16 + 8 < 2 ** 24
    return c


@pytest.mark.parametrize("args", [("conv", 33, 65, 7, 130, 1, 3, 9, 0), ("conv", 9, 5, 4, 131, 2, 1, 1, 0), ("conv", 40, 64, 1, 65, 1, 1, 0, 0),
                                  ("convt", 17, 65, 16, 20, 8, 1, 4, 0), ("convt", 33, 5, 10, 27, 5, 1, 3, 1), ("convt", 9, 64, 4, 70, 2, 1, 1, 0)],
                         ids=lambda a: "_".join(str(v) for v in a))
def test_small_integers_are_exact(dev, args):
    """every partial sum is an integer below 2^24, so any correct fp32 evaluation equals the float64 convolution bit for bit"""
    c = _int_case(*args, seed=sum(args[1:]))
    y = launch_full(c, dev).cpu()
    assert same_bits(y, c["ref"].float()), (c["name"], float((y.double() - c["ref"]).abs().max()))


# ================================================================================================ windows and rows
@pytest.mark.parametrize("kind", ["conv", "convt"])
def test_windows_and_rows_are_bit_identical_to_the_full_launch(dev, kind):
    st = Stats()
    groups = CONV_GROUPS if kind == "conv" else CONVT_GROUPS
    cases = [conv_case(s["name"], sn) for grp in groups.values() for s in grp for sn in s["snakes"]] + cases_of(EDGE[kind])
    wins = rows = 0
    for c in cases:
        ws = windows_of(c["Lout"])
        if not ws:
            continue
        full = launch_full(c, dev).cpu()
        bufs = [win_buffers(c, t0, n) for t0, n in ws]
        for wb in bufs:
            y = launch_win(c, wb, dev).cpu()
            check_win(c, wb, y, st, kind + " windows")
            lo = wb["t0"] - wb["y_off"]
            assert same_bits(y[:, :, lo:lo + wb["n"]], full[:, :, wb["t0"]:wb["t0"] + wb["n"]]), (c["name"], wb["t0"], wb["n"])
            wins += 1
        # rows: batch plane 0 and batch plane 2 on different windows (t_begin 61 / 1 / Lout - 3 are no multiples of the tile), row 1 idle
        for wa, wc in ((bufs[1], bufs[2]), (bufs[3], bufs[0])):
            ys = launch_rows(c, [(0, wa), None, (2, wc)], dev)
            for (b, wb), y in (((0, wa), ys[0]), ((2, wc), ys[2])):
                y = y.cpu()
                lo, n, t0 = wb["t0"] - wb["y_off"], wb["n"], wb["t0"]
                assert same_bits(y[:, lo:lo + n], full[b, :, t0:t0 + n]), (c["name"], b, t0, n)
                inside = torch.zeros(y.shape, dtype=torch.bool)
                inside[:, lo:lo + n] = True
                keeps_sentinel(f"{c['name']} row window [{t0}, {t0 + n}): y outside the window", y[~inside])
            rows += 1
    assert wins >= 60 and rows >= 30, (wins, rows)
    st.show(f"mfma {kind} ({wins} window launches, {rows} row launches)")


def test_idle_rows_are_accepted_and_write_nothing(dev):
    """all rows idle (n = 0; their other words, here valid planes, are not to be used), with max_n = 0 (the entry returns before the
    launch) and with max_n > 0 (workgroups start and leave): both succeed and no plane is touched.  (Whether a launch was enqueued
    cannot be seen from here; the max_n == 0 return is read in the entry's code.)"""
    from unimoe_audio_amd.dac import dac_row_words
    x = torch.randn(2, 20, device=dev)
    y = torch.full((2, 3, 16), SENT, device=dev)
    host = torch.tensor([dac_row_words(x=x.data_ptr(), y=y[r].data_ptr(), Lx=20, Ly=16, L=20) for r in range(2)], dtype=torch.int64)
    table = host.to(dev)
    w = torch.ones(64, device=dev)
    for max_n in (0, 5, 200):
        assert lib().umoe_dac_conv1d_win_rows_mfma(_p(host), _p(table), 2, max_n, _p(w), None, None, 2, 3, 3, 1, 1, 1, 0, _stream()) == 0, last_error()
        assert lib().umoe_dac_conv_transpose1d_win_rows_mfma(_p(host), _p(table), 2, max_n, _p(w), None, None, 2, 3, 4, 2, 1, 0, _stream()) == 0, last_error()
    torch.cuda.synchronize()
    keeps_sentinel("idle rows", y.cpu())


# ================================================================================================ refusals
def test_refusals_write_nothing(dev):
    from unimoe_audio_amd import _lib as L, dac as D
    from unimoe_audio_amd.dac import dac_row_words
    lb = lib()
    x = torch.randn(1, 8, 600, device=dev)
    wt = torch.randn(8, 32, 8, device=dev)
    y = torch.full((4096,), SENT, device=dev)
    st = _stream()

    def refused(rc, *words):
        msg = last_error()
        assert rc != 0 and all(w in msg for w in words), (rc, msg, words)

    # bad arguments, one at a time (the direct siblings' lists)
    good = dict(x=_p(x), wt=_p(wt), B=1, Cin=8, L=100, Cout=8, K=3, stride=1, dil=1, pad=1, y=_p(y))
    for k, v in (("x", None), ("wt", None), ("y", None), ("B", 0), ("Cin", 0), ("Cout", 0), ("K", 0), ("stride", 0), ("dil", 0), ("pad", -1), ("L", 0)):
        a = dict(good, **{k: v})
        lo = C.c_int(-1)
        refused(lb.umoe_dac_conv1d_mfma(a["x"], a["wt"], None, None, None, a["B"], a["Cin"], a["L"], a["Cout"], a["K"], a["stride"], a["dil"], a["pad"], 0,
                                        a["y"], C.byref(lo), st), "umoe_dac_conv1d_mfma", "bad argument")
        assert lo.value == -1
        if k != "dil":
            refused(lb.umoe_dac_conv_transpose1d_mfma(a["x"], a["wt"], None, None, a["B"], a["Cin"], a["L"], a["Cout"], a["K"], a["stride"], a["pad"], 0,
                                                      a["y"], C.byref(lo), st), "umoe_dac_conv_transpose1d_mfma", "bad argument")
        refused(lb.umoe_dac_conv1d_win_mfma(a["x"], 0, 100, a["wt"], None, None, None, 0, 0, a["B"], a["Cin"], a["L"], a["Cout"], a["K"], a["stride"],
                                            a["dil"], a["pad"], 0, 0, 4, a["y"], 0, 64, st), "umoe_dac_conv1d_win_mfma", "bad argument")
        if k != "dil":
            refused(lb.umoe_dac_conv_transpose1d_win_mfma(a["x"], 0, 100, a["wt"], None, None, a["B"], a["Cin"], a["L"], a["Cout"], a["K"], a["stride"],
                                                          a["pad"], 0, 0, 4, a["y"], 0, 64, st), "umoe_dac_conv_transpose1d_win_mfma", "bad argument")
    refused(lb.umoe_dac_conv_transpose1d_mfma(_p(x), _p(wt), None, None, 1, 8, 100, 8, 4, 2, 1, -1, _p(y), None, st), "bad argument")
    refused(lb.umoe_dac_conv_transpose1d_mfma(_p(x), _p(wt), None, None, 1, 8, 1, 8, 2, 2, 1, 0, _p(y), None, st), "empty output")
    for k, v in (("Lx", 0), ("Ly", 0), ("t_begin", -1), ("n", 0)):
        a = dict(dict(Lx=100, Ly=64, t_begin=0, n=4), **{k: v})
        refused(lb.umoe_dac_conv1d_win_mfma(_p(x), 0, a["Lx"], _p(wt), None, None, None, 0, 0, 1, 8, 100, 8, 3, 1, 1, 1, 0, a["t_begin"], a["n"], _p(y), 0,
                                            a["Ly"], st), "bad argument")
        refused(lb.umoe_dac_conv_transpose1d_win_mfma(_p(x), 0, a["Lx"], _p(wt), None, None, 1, 8, 100, 8, 4, 2, 1, 0, a["t_begin"], a["n"], _p(y), 0,
                                                      a["Ly"], st), "bad argument")
    # every empty output of the float64 file's grid
    for (Lx, K, d, s, p) in F64.empty_geometries():
        lo = C.c_int(-1)
        refused(lb.umoe_dac_conv1d_mfma(_p(x), _p(wt), None, None, None, 1, 2, Lx, 3, K, s, d, p, 0, _p(y), C.byref(lo), st), "empty output")
        assert lo.value == -1
        refused(lb.umoe_dac_conv1d_win_mfma(_p(x), 0, Lx, _p(wt), None, None, None, 0, 0, 1, 2, Lx, 3, K, s, d, p, 0, 0, 1, _p(y), 0, 64, st), "empty output")
    for (Lx, K, s, p) in ((2, 3, 2, 0), (1, 4, 3, 1), (1, 7, 1, 0)):
        with pytest.raises(L.UmoeError, match="empty output"):
            D.conv1d(x[:, :2, :Lx].contiguous(), torch.randn(3, 2, K, device=dev), None, stride=s, padding=p, form="mfma")
    with pytest.raises(ValueError):
        D.conv1d(x, torch.randn(3, 8, 3, device=dev), None, form="bf16")
    with pytest.raises(ValueError):
        D.conv_transpose1d(x, torch.randn(8, 3, 4, device=dev), None, stride=2, padding=1, form="MFMA")
    with pytest.raises(L.UmoeError, match="contiguous float32 device"):
        D.conv1d(x.cpu(), torch.randn(3, 8, 3), None, form="mfma")
    # the windows' own checks (L 100, K 3, pad 1: Lout 100; transposed L 100, K 4, stride 2, pad 1: Lout 200)
    conv_w = lambda **k: lb.umoe_dac_conv1d_win_mfma(_p(x), k.get("x_off", 0), k.get("Lx", 100), _p(wt), None, None, k.get("r"), k.get("r_off", 0),      # noqa: E731
                                                     k.get("Lr", 0), 1, 8, 100, 8, 3, 1, 1, 1, 0, k.get("t0", 0), k.get("n", 4), _p(y), k.get("y_off", 0),
                                                     k.get("Ly", 64), st)
    convt_w = lambda **k: lb.umoe_dac_conv_transpose1d_win_mfma(_p(x), k.get("x_off", 0), k.get("Lx", 100), _p(wt), None, None, 1, 8, 100, 8, 4, 2, 1, 0,      # noqa: E731
                                                                k.get("t0", 0), k.get("n", 4), _p(y), k.get("y_off", 0), k.get("Ly", 64), st)
    refused(conv_w(t0=98, n=3), "past the sequence")
    refused(convt_w(t0=198, n=3), "past the sequence")
    refused(conv_w(t0=50, n=4, x_off=50, Lx=20, y_off=50), "read input")
    refused(conv_w(t0=50, n=4, x_off=40, Lx=13, y_off=50), "read input")
    refused(convt_w(t0=100, n=4, x_off=51, Lx=20, y_off=100), "read input")
    refused(conv_w(t0=10, n=4, y_off=11), "output buffer")
    refused(conv_w(t0=10, n=60, y_off=10, Ly=59), "output buffer")
    refused(convt_w(t0=10, n=4, y_off=8, Ly=5), "output buffer")
    refused(conv_w(t0=10, n=4, r=_p(y), r_off=11, Lr=20), "residual buffer")
    refused(conv_w(t0=10, n=4, r=_p(y), r_off=0, Lr=13), "residual buffer")
    # tables
    row = lambda **k: dac_row_words(**dict(dict(x=x.data_ptr(), y=y.data_ptr(), Lx=100, Ly=64, n=4, L=100), **k))      # noqa: E731

    def conv_r(words, max_n=8, rows=None, table=None, host=True):
        h = torch.tensor(words, dtype=torch.int64)
        t = h.to(dev)
        return lb.umoe_dac_conv1d_win_rows_mfma(_p(h) if host else None, table if table is not None else _p(t), len(words) if rows is None else rows,
                                                max_n, _p(wt), None, None, 8, 8, 3, 1, 1, 1, 0, st)

    def convt_r(words, max_n=8):
        h = torch.tensor(words, dtype=torch.int64)
        t = h.to(dev)
        return lb.umoe_dac_conv_transpose1d_win_rows_mfma(_p(h), _p(t), len(words), max_n, _p(wt), None, None, 8, 8, 4, 2, 1, 0, st)

    refused(conv_r([row()], host=False), "bad argument")
    refused(conv_r([row()], rows=0), "bad argument")
    refused(conv_r([row()], max_n=-1), "bad argument")
    refused(conv_r([row()], table=C.c_void_p(y.data_ptr() + 4)), "8-byte aligned")
    refused(conv_r([row(), row(n=9)]), "row 1 has n = 9")
    refused(conv_r([row(), row(x=0)]), "null plane")
    refused(conv_r([row(), row(x_off=-1)]), "not a non-negative int")
    refused(conv_r([row(), row(L=1 << 31)]), "not a non-negative int")
    refused(conv_r([dac_row_words(), row(t_begin=98)]), "past the sequence")
    refused(conv_r([row(t_begin=50, x_off=50, Lx=20, y_off=50)]), "read input")
    refused(convt_r([row(), row(n=9)]), "row 1 has n = 9")
    refused(convt_r([row(), row(y=0)]), "null plane")
    refused(convt_r([row(t_begin=198, y_off=198)]), "past the sequence")
    refused(convt_r([row(t_begin=10, y_off=8, Ly=5)]), "output buffer")
    # what these kernels cannot launch: their own limit (no LDS refusal: the staging images are fixed)
    lo = C.c_int(-1)
    refused(lb.umoe_dac_conv1d_mfma(_p(x), _p(wt), None, None, None, 1, 8, 100, 64 * 65535 + 1, 3, 1, 1, 1, 0, _p(y), C.byref(lo), st), "launch limits")
    assert lo.value == -1
    refused(lb.umoe_dac_conv1d_mfma(_p(x), _p(wt), None, None, None, 65536, 8, 100, 8, 3, 1, 1, 1, 0, _p(y), None, st), "launch limits")
    refused(lb.umoe_dac_conv_transpose1d_mfma(_p(x), _p(wt), None, None, 65536, 8, 100, 8, 4, 2, 1, 0, _p(y), None, st), "launch limits")
    refused(lb.umoe_dac_conv1d_win_mfma(_p(x), 0, 100, _p(wt), None, None, None, 0, 0, 1, 1 << 30, 100, 8, 3, 1, 1, 1, 0, 0, 4, _p(y), 0, 64, st),
            "does not fit an int")
    torch.cuda.synchronize()
    keeps_sentinel("refused launches", y.cpu())


# ================================================================================================ model level
@pytest.fixture(scope="module")
def small_model(dev):
    """the model of tests/test_gpu_dac.py: the 16 kHz geometry with narrower channels, residual branches and the head damped"""
    from unimoe_audio_amd import dac as D
    m = D.DacModel(encoder_dim=16, encoder_rates=[2, 4, 5, 8], decoder_dim=192, decoder_rates=[8, 5, 4, 2], n_codebooks=12, codebook_size=1024,
                   codebook_dim=8).init_random(3)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("block.3.weight_g"):
                p.mul_(0.15)
            if n == "decoder.model.6.weight_g":
                p.mul_(0.05)
    return m.to(dev).float()


def test_model_in_mfma_vs_torch_walk_and_direct_unchanged(dev, small_model):
    from test_gpu_dac import close, torch_graph
    from unimoe_audio_amd import dac as D
    gm = small_model
    assert gm.conv_form == "direct"
    f = gm._folded()
    assert f["wt"] == {}
    f_cpu = {k: (tuple(t.cpu() for t in v) if isinstance(v, tuple) else v.cpu()) for k, v in f.items() if not isinstance(k, str)}
    g = torch.Generator().manual_seed(4)
    x = gm.preprocess(0.3 * torch.randn(1, 1, 320 * 40 - 57, generator=g))
    z_d, codes_d = gm.encode(x.to(dev))
    wav_d = gm.decode(gm.from_codes(codes_d))
    gm.set_conv_form("mfma")
    try:
        fm = gm._folded()
        convs = [m for part in (gm.encoder, gm.decoder) for m in part.modules() if isinstance(m, D._WN)]
        assert set(fm["wt"]) == {m for m in convs if D.uses_mfma(*m.shape4())} and fm["wt"]
        z, codes = gm.encode(x.to(dev))
        z_ref = torch_graph(gm, f_cpu, x, gm.encoder.items())
        assert z.shape == z_ref.shape == (1, 256, 40) and close(z.cpu(), z_ref, 5e-4)
        assert not same_bits(z, z_d)                          # (another summation order: the MFMA path did run)
        res = z[0].cpu().double().t().clone()
        cb, in_w, in_b, out_w, out_b = (fm[k].cpu().double() for k in ("cb", "in_w", "in_b", "out_w", "out_b"))
        for q in range(12):
            e = res @ in_w[q].t() + in_b[q]
            sim = F.normalize(e, dim=-1) @ F.normalize(cb[q], dim=-1).t()
            top2 = sim.topk(2, dim=-1)
            clear = (top2.values[:, 0] - top2.values[:, 1]) > 1e-5
            assert torch.equal(codes[0, q].cpu()[clear], top2.indices[:, 0][clear]), q
            res = res - cb[q][codes[0, q].cpu()] @ out_w[q].t() - out_b[q]
        zq = gm.from_codes(codes_d)
        wav = gm.decode(zq)
        wav_ref = torch_graph(gm, f_cpu, zq.cpu(), gm.decoder.items())
        assert wav.shape == wav_ref.shape == wav_d.shape
        assert 0.01 < float(wav_ref.abs().max()) < 0.999
        assert close(wav.cpu(), wav_ref, 1e-3)
        assert not same_bits(wav, wav_d)
    finally:
        gm.set_conv_form("direct")
    # back in "direct": today's bytes
    z2, codes2 = gm.encode(x.to(dev))
    assert gm._folded()["wt"] == {}
    assert same_bits(z2, z_d) and torch.equal(codes2, codes_d) and same_bits(gm.decode(gm.from_codes(codes_d)), wav_d)


def _routed_as_the_predicate_says(model, names):
    """the library calls of a run in "mfma": MFMA entries, and direct conv entries only if dac.uses_mfma keeps some layer on them"""
    from unimoe_audio_amd import dac as D
    convs = [n for n in names if "dac_conv" in n]
    some_direct = any(not D.uses_mfma(*m.shape4()) for part in (model.encoder, model.decoder) for m in part.modules() if isinstance(m, D._WN))
    assert any(n.endswith("_mfma") for n in convs), sorted(set(convs))
    assert some_direct or all(n.endswith("_mfma") for n in convs), sorted(set(convs))


def test_stream_decoders_in_mfma_are_bit_identical_to_decode(dev):
    from tests.test_serve_stream_cpu import _drive, _with_window_log
    from unimoe_audio_amd import dac as D
    dm = D.DacModel(encoder_dim=16, decoder_dim=192).init_random(5).to(dev).float().set_conv_form("mfma")
    calls, lib_call = [], D._lib_call
    # DacStreamDecoder, one row, an uneven schedule
    g = torch.Generator().manual_seed(11)
    z = torch.randn(1, dm.latent_dim, 41, generator=g).to(dev)

    def source(rows, f0, n, out, col):
        out[:, :, col:col + n] = z[rows][:, :, f0:f0 + n]

    dec = D.DacStreamDecoder(dm, 1, source)
    parts = [dec.push(n)[0] for n in (1, 7, 3, 16, 13, 1)]
    parts.append(dec.flush([0])[0])
    ref = dm.decode(z)[0, 0]
    assert same_bits(torch.cat(parts), ref)
    # DacRowStreamDecoder: ragged and grouped, rows starting at different pushes, flushes, a reset and a reused row
    waves = {}
    for ragged in (True, False):
        rd = _with_window_log(D.DacRowStreamDecoder)(dm, 3, None, max_frames=25, ragged=ragged)
        rd.wlog, rd.z = [], {}

        def src(requests, slab, rd=rd):
            for row, f0, n, col in requests:
                slab[row, :, col:col + n] = rd.z[row][:, f0:f0 + n].to(slab)

        rd.source = src
        for b in rd.bufs:
            b.fill_(float("nan"))
        D._lib_call = lambda name, *a: (calls.append(name), lib_call(name, *a))[1]
        try:
            waves[ragged] = _drive(rd, dm)
        finally:
            D._lib_call = lib_call
    assert sorted(waves[True]) == [(0, 0), (1, 0), (2, 0), (2, 1)]
    for key, (wave, zz) in waves[True].items():
        ref = dm.decode(zz.float().to(dev)[None])[0, 0]
        assert same_bits(wave, ref), key
        assert same_bits(wave, waves[False][key][0]), key
    _routed_as_the_predicate_says(dm, calls)


def test_serve_stream_equals_serve_with_an_mfma_codec(dev, tmp_path, monkeypatch):
    from tests.test_gpu_serve_stream import _requests, _serve_both
    from tests.test_gpu_stream import _app, _tiny_model
    from unimoe_audio_amd import dac as D
    m = _tiny_model(dev)
    app = _app(m, dev)
    reqs = _requests(tmp_path)
    kw = dict(slots=3, poll_every=8, max_prompt_tokens=256, max_audio_seconds=2, use_graph=False, prefix_cache=True)
    app.dac = D.Dac(model=app.dac.model, conv_form="mfma")
    assert app.dac.conv_form == "mfma"
    names, lib_call = [], D._lib_call
    monkeypatch.setattr(D, "_lib_call", lambda name, *a: (names.append(name), lib_call(name, *a))[1])
    _serve_both(app, reqs, tmp_path, "mfma", monkeypatch, **kw)
    _routed_as_the_predicate_says(app.dac.model, names)
    m._engine.close()
    m._engine = None
