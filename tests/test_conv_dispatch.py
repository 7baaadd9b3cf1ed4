"""The conv dispatch layer of csl_gan_amd.ops asks the library for exactly what it asked before it was rewritten — checked without a GPU.

scripts/conv_dispatch_log.py drives the layer on zero-filled CPU tensors against a recording stand-in for the library.
tests/conv_dispatch_calls.json holds, per case, the ordered entry names and a SHA-1 of the canonical JSON of the full log (entry, every
scalar argument, every descriptor field, where each pointer points, repack-cache requests, timer records, the returned tensor),
recorded from the commit BEFORE the layer was rewritten around one geometry record.  It is never re-recorded from later code: a log
that differs is a change of behaviour.  tests/test_kernel_routes_gpu.py pins the other half, the kernel the library then picks."""
import importlib.util
import json
import os

import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("conv_dispatch_log", os.path.join(_ROOT, "scripts", "conv_dispatch_log.py"))
dispatch_log = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dispatch_log)

with open(os.path.join(_ROOT, "tests", "conv_dispatch_calls.json")) as _f:
    FIXTURE = json.load(_f)

# the twenty cslgan_conv2d_* entries and the two bf16-stored head entries the conv section calls
CONV_ENTRIES = [
    "cslgan_conv2d_c3_fwd_bf16out", "cslgan_conv2d_c3_wgrad_bf16gy", "cslgan_conv2d_dgrad_bf16s", "cslgan_conv2d_dgrad_f32",
    "cslgan_conv2d_dgrad_skinny_bf16in", "cslgan_conv2d_dgrad_x3_f32", "cslgan_conv2d_fwd_bf16s", "cslgan_conv2d_fwd_f32",
    "cslgan_conv2d_fwd_skinny_bf16in", "cslgan_conv2d_fwd_x3_f32", "cslgan_conv2d_s2_fwd_f32", "cslgan_conv2d_s2_fwd_x3_f32",
    "cslgan_conv2d_wgrad_blocks_f32", "cslgan_conv2d_wgrad_grouped_bf16out_f32", "cslgan_conv2d_wgrad_grouped_bf16s",
    "cslgan_conv2d_wgrad_grouped_f32", "cslgan_conv2d_wgrad_scaled_bf16s", "cslgan_conv2d_wgrad_scaled_f32",
    "cslgan_conv2d_wgrad_skinny_f32", "cslgan_conv2d_wgrad_sqnorm_gram_f32", "cslgan_linear_k1_dgrad_bf16s", "cslgan_linear_k1_wgrad_bf16s",
]


@pytest.fixture
def harness(monkeypatch):
    return dispatch_log.Harness(monkeypatch.setattr)


def test_fixture_covers_every_case():
    assert set(FIXTURE) == set(dispatch_log.CASES)
    assert len(FIXTURE) >= 100


def test_every_conv_entry_is_reached():
    reached = {e for rec in FIXTURE.values() for e in rec["entries"] if dispatch_log.is_conv_entry(e)}
    assert sorted(reached) == CONV_ENTRIES == dispatch_log.CONV_ENTRIES


def test_every_exported_conv_entry_is_listed():
    from csl_gan_amd import _lib
    assert sorted(e for e in _lib.EXPORTS if dispatch_log.is_conv_entry(e)) == CONV_ENTRIES


def _groups():
    """Case names by their prefix (fwd, dgrad, wgrad, ...): one test per group keeps the per-test fixtures of this suite off hundreds of items."""
    groups = {}
    for name in dispatch_log.CASES:
        groups.setdefault(name.split("_")[0], []).append(name)
    return groups


@pytest.mark.parametrize("group", sorted(_groups()))
def test_call_logs(harness, group):
    """For every case the log equals the recorded one; a mismatch prints the full current log."""
    bad = []
    for name in _groups()[group]:
        log = harness.log(name)
        if dispatch_log.entries(log) != FIXTURE[name]["entries"] or dispatch_log.digest(log) != FIXTURE[name]["sha1"]:
            bad.append("%s: recorded entries %s, current log\n%s" % (name, FIXTURE[name]["entries"], json.dumps(log, indent=1, sort_keys=True)))
        assert (log["error"] == "RuntimeError") == name.startswith("err_"), name        # err_* cases raise, no other case does
    assert not bad, "\n\n".join(bad)


def test_untimed_path_makes_the_same_calls(monkeypatch):
    """No launch timer installed (the product path): the same calls, and no tag is formatted."""
    h = dispatch_log.Harness(monkeypatch.setattr, timer=False)
    for name in dispatch_log.CASES:
        log = h.log(name)
        assert dispatch_log.entries(log) == FIXTURE[name]["entries"] and log["timed"] == [], name
