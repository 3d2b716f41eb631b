"""GPU tests of prefix reuse across admissions.  The cases are in tests/prefix_gpu_cases.py; each test here runs one group
of them in a child process and fails with the child's output if any case fails.

  kernel, geometry, refusals, serve   umoe_kv_prefix_copy bit for bit against sentinel slabs (P 1, 63, 64, 65; pads 0, 3, > P; refused
                                      ranges); build -> admit behind the store at P on both sides of the tiled threshold: the installed
                                      slots hold the store, nothing else of the cache changes; a one-token prefix against token 0 of a
                                      longer one; refusals that enqueue nothing; serve(prefix_cache=True): 2 misses, 4 hits, every
                                      request's codes those of the request served as the only one of its voice; an engine held while its
                                      model is dropped
  hit equals miss                     a request behind a store built in the admission (idle engine, step 0) and behind one built earlier
                                      through another row, admitted at step 7 beside three decoding rows: same store, K / V, codes and
                                      length, eager and graph with one capture, bf16 and fp8; the other rows undisturbed; row reuse
  against the one-shot admission      first-step logits within 2x the tiled-against-ragged yardstick, routing masks of every layer equal

Why children: the cases build models and engines of several sizes and empty torch's caching allocator as they go, and the suite's
process carries that allocator from file to file.  A child leaves it as it found it."""
import os
import subprocess
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "prefix_gpu_cases.py")
LIMIT = 300          # seconds per child: a group takes 5 to 10 s on an idle MI355X, interpreter start included; the limit is for a hang
_stopped = []        # why no further child is started: a child that hit its limit or died of a signal may have left the GPU in trouble


def _child(k_expr):
    """one pytest child on the cases file.  A child that fails, dies of a signal or runs into its time limit fails the caller with its
    output and is not run again; after a child that did not end as a pytest run ends, no other child is started."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no GPU is visible")
    if _stopped:
        pytest.fail(f"not started: {_stopped[0]}")
    t = time.time()
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", CASES, "-q", "-s", "-x", "-m", "gpu", "-k", k_expr, "-p", "no:cacheprovider"],
                           env=dict(os.environ), capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired as e:
        _stopped.append(f"the child '{k_expr}' ran into its time limit of {LIMIT} s")
        pytest.fail(f"{_stopped[0]}:\n{str(e.stdout)[-3000:]}")
    if r.returncode not in (0, 1):           # (0 all passed, 1 some case failed; anything else: a signal, an abort, a usage or internal error)
        _stopped.append(f"the child '{k_expr}' ended with status {r.returncode}")
    assert r.returncode == 0, f"child '{k_expr}' returned {r.returncode} after {time.time() - t:.0f} s:\n" + r.stdout[-6000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert " passed" in last and "skipped" not in last and "no tests ran" not in r.stdout, r.stdout[-1500:]
    print(f"\nPREFIX CHILD '{k_expr}' {time.time() - t:.0f} s: {last}")
    for line in r.stdout.splitlines():
        if line.startswith(("split admission:", "served_prefix", "one-token prefix:")) or " p miss length " in line:
            print("  " + line)


def test_kernel_geometry_refusals_serve_and_engine_lifetime():
    _child("install_and_extract or build_install_geometry or one_token_prefix or refusals or serve_with or model_is_dropped")


def test_hit_equals_miss_undisturbed_rows_and_row_reuse():
    _child("hit_equals_miss or does_not_disturb or reused_row")


def test_split_admission_against_the_one_shot_admission():
    _child("split_admission")
