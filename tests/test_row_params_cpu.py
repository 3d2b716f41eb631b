"""CPU suite of the per-request settings table (umoe_row_params): the C layout against its ctypes mirror and the numpy dtype the host
packs, the new export, and the host-side packing (unimoe_audio_amd/row_params.py) -- no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _header():
    txt = open(os.path.join(ROOT, "include", "umoe.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_row_params_mirror_has_the_c_layout(tmp_path):
    from unimoe_audio_amd import _lib as L
    from unimoe_audio_amd.row_params import ROW_DTYPE
    cls = L.TABLE_MIRRORS["umoe_row_params"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "umoe.h"', 'int main(void) {',
           '  printf("size %zu\\n", sizeof(umoe_row_params));']
    for fname, _ in cls._fields_:
        src.append(f'  printf("{fname} %zu\\n", offsetof(umoe_row_params, {fname}));')
    src += ['  printf("sample.row_params %zu %zu\\n", offsetof(umoe_sample_args, row_params), sizeof(umoe_sample_args));',
            '  printf("io.row_params %zu %zu\\n", offsetof(umoe_decode_io, row_params), sizeof(umoe_decode_io));', '  return 0;', '}']
    cfile, exe = tmp_path / "probe.c", tmp_path / "probe"
    cfile.write_text("\n".join(src))
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)])
    got = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in subprocess.check_output([str(exe)], text=True).splitlines()}
    assert got["size"] == [40] and C.sizeof(cls) == 40 and ROW_DTYPE.itemsize == 40
    want = dict(cfg_scale=0, temperature=4, top_p=8, eos_mul=12, top_k=16, do_sample=20, min_tokens=24, max_tokens=28, seed=32)
    assert [n for n, _ in cls._fields_] == list(want) and list(ROW_DTYPE.names) == list(want)
    for fname, off in want.items():
        assert got[fname] == [off], fname
        assert getattr(cls, fname).offset == off, fname
        assert ROW_DTYPE.fields[fname][1] == off, fname
        assert ROW_DTYPE.fields[fname][0].itemsize == C.sizeof(dict(cls._fields_)[fname]), fname
    # the pointer is the LAST member of both argument structs, and the mirrors put it where the header does
    for key, mirror in (("sample.row_params", L.SampleArgs), ("io.row_params", L.DecodeIO)):
        off, size = got[key]
        assert mirror._fields_[-1][0] == "row_params" and mirror.row_params.offset == off and C.sizeof(mirror) == size
        assert off + 8 == size
    # the built library was compiled with the same record (checked at every load, too)
    assert int(L.lib().umoe_struct_size(b"umoe_row_params")) == 40


def test_delay_step_rows_is_exported_and_declared():
    from unimoe_audio_amd import _lib as L
    assert re.search(r"\bumoe_delay_step_rows\s*\(", _header())
    assert "umoe_delay_step_rows" in L.EXPORTS
    lib = C.CDLL(L.build())
    assert hasattr(lib, "umoe_delay_step_rows") and hasattr(lib, "umoe_delay_step")
    # umoe_delay_step keeps its signature: the declaration has no table argument
    m = re.search(r"int umoe_delay_step\((.*?)\);", _header(), flags=re.S)
    assert m and "row_params" not in m.group(1)
    m = re.search(r"int umoe_delay_step_rows\((.*?)\);", _header(), flags=re.S)
    assert m and re.search(r"const umoe_row_params\*\s*row_params,\s*umoe_stream_t stream$", " ".join(m.group(1).split()))


SCALARS = dict(cfg_scale=3.0, temperature=1.2, top_p=0.95, top_k=45, eos_mul=0.8, do_sample=True, seed=7, min_tokens=100, max_tokens=500)


def test_scalars_only_pack_no_table():
    from unimoe_audio_amd.row_params import pack_row_params
    assert pack_row_params(4, **SCALARS) is None
    assert pack_row_params(1, **dict(SCALARS, top_k=None, min_tokens=None)) is None
    assert pack_row_params(4, **dict(SCALARS, seed=np.int64(3), temperature=np.float32(1.0))) is None      # 0-d values are scalars


def test_a_sequence_broadcasts_the_rest_and_lands_in_its_field():
    import torch
    from unimoe_audio_amd.row_params import ROW_DTYPE, SETTINGS, pack_row_params
    per_row = dict(cfg_scale=[0.0, 1.0, 3.0, 10.0], temperature=(0.3, 1.0, 1.2, 2.0), top_p=np.array([0.5, 0.95, 1.0, 1.0]),
                   top_k=[1, 64, 65, None], eos_mul=[0.6, 0.8, 1.0, 3.0], do_sample=[True, False, True, True],
                   seed=[0, 1, 2 ** 63 + 5, 2 ** 64 - 1], min_tokens=[None, 0, 100, 400], max_tokens=torch.tensor([150, 500, 1000, 50]))
    assert set(per_row) == set(SETTINGS)
    want = dict(per_row, top_k=[1, 64, 65, -1], min_tokens=[-1, 0, 100, 400], do_sample=[1, 0, 1, 1], max_tokens=[150, 500, 1000, 50])
    for name in SETTINGS:                                         # one sequence at a time: the others are broadcast
        t = pack_row_params(4, **dict(SCALARS, **{name: per_row[name]}))
        assert t.dtype == ROW_DTYPE and t.shape == (4,)
        for other in SETTINGS:
            if other == name:
                exp = np.array(want[name], dtype=ROW_DTYPE.fields[name][0])
            else:
                exp = np.full(4, int(SCALARS[other]) if other == "do_sample" else SCALARS[other]).astype(ROW_DTYPE.fields[other][0])
            assert np.array_equal(t[other], exp), (name, other, t[other], exp)
    t = pack_row_params(4, **per_row)                             # all at once
    for name in SETTINGS:
        assert np.array_equal(t[name], np.array(want[name], dtype=ROW_DTYPE.fields[name][0])), name
    # the bytes are the C records: entry b, field by field, through the ctypes mirror
    from unimoe_audio_amd import _lib as L
    raw = np.ascontiguousarray(t).view(np.uint8).tobytes()
    assert len(raw) == 4 * 40
    for b in range(4):
        rec = L.RowParams.from_buffer_copy(raw[40 * b: 40 * b + 40])
        assert rec.seed == want["seed"][b] and rec.top_k == want["top_k"][b] and rec.max_tokens == want["max_tokens"][b]
        assert rec.min_tokens == want["min_tokens"][b] and rec.do_sample == want["do_sample"][b]
        assert rec.temperature == np.float32(want["temperature"][b]) and rec.top_p == np.float32(want["top_p"][b])
        assert rec.cfg_scale == np.float32(want["cfg_scale"][b]) and rec.eos_mul == np.float32(want["eos_mul"][b])
    # top_k / min_tokens None as a SCALAR beside a sequence, and negative seeds wrap like the C cast
    t = pack_row_params(2, **dict(SCALARS, top_k=None, min_tokens=None, seed=[-1, 5]))
    assert t["top_k"].tolist() == [-1, -1] and t["min_tokens"].tolist() == [-1, -1] and t["seed"].tolist() == [2 ** 64 - 1, 5]


@pytest.mark.parametrize("name", ["cfg_scale", "temperature", "top_p", "top_k", "eos_mul", "do_sample", "seed", "min_tokens", "max_tokens"])
def test_wrong_length_raises_naming_the_argument(name):
    from unimoe_audio_amd._lib import UmoeError
    from unimoe_audio_amd.row_params import pack_row_params
    for n in (0, 3, 5):
        with pytest.raises(UmoeError, match=rf"^{name}: a sequence of {n} values for a batch of 4"):
            pack_row_params(4, **dict(SCALARS, **{name: [1] * n}))
    with pytest.raises(TypeError):
        pack_row_params(4, **{k: v for k, v in SCALARS.items() if k != name})


def test_none_is_only_a_value_of_top_k_and_min_tokens():
    from unimoe_audio_amd._lib import UmoeError
    from unimoe_audio_amd.row_params import pack_row_params
    with pytest.raises(UmoeError, match="temperature"):
        pack_row_params(2, **dict(SCALARS, temperature=[1.0, None]))


def test_helpers_for_sizes_and_seconds():
    from unimoe_audio_amd.row_params import is_sequence, largest, scaled
    assert largest(500) == 500 and largest([150, 1000, 50]) == 1000 and largest(np.array([3, 9])) == 9
    assert scaled(10, 50) == 500 and scaled([3, 10], 50) == [150, 500]
    assert not is_sequence("abc") and not is_sequence(None) and not is_sequence(np.float32(1)) and is_sequence(())


def test_request_defaults_are_the_task_methods_defaults():
    """SpeechRequest / MusicRequest carry the defaults of text_to_speech / text_to_music (plus seed)"""
    import dataclasses
    import inspect
    from unimoe_audio_amd.api import MusicRequest, SpeechRequest, UniMoEAudio
    for req, fn in ((SpeechRequest, UniMoEAudio.text_to_speech), (MusicRequest, UniMoEAudio.text_to_music)):
        sig = inspect.signature(fn).parameters
        seen = 0
        for f in dataclasses.fields(req):
            if f.default is dataclasses.MISSING:
                continue
            assert f.name in sig, (req.__name__, f.name)
            assert sig[f.name].default == f.default, (req.__name__, f.name, sig[f.name].default, f.default)
            seen += 1
        assert seen >= 10 and "seed" in {f.name for f in dataclasses.fields(req)}
