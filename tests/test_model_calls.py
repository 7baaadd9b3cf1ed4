"""The model layer (csl_gan_amd.nn, DCResNet_models, the conv Functions of functional, the normalisation wrappers of ops) launches
exactly what it launched before it was rewritten around one route per norm / conv stage — checked without a GPU.

scripts/model_call_log.py runs whole generators and critics on zero-filled CPU tensors against a recording stand-in for the library.
tests/model_calls.json holds, per case, the ordered library entries and a SHA-1 of the canonical JSON of the full log (every library
call with its scalars, struct fields and where each pointer points — parameter, input or the ordinal of the tensor's first appearance,
i.e. the data flow between the launches —, the ATen operators in between, what the call returned and the .grad it left), recorded from
the commit BEFORE that rewrite.  It is never re-recorded from later code: a log that differs is a change of behaviour."""
import importlib.util
import json
import os

import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("model_call_log", os.path.join(_ROOT, "scripts", "model_call_log.py"))
call_log = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(call_log)

with open(os.path.join(_ROOT, "tests", "model_calls.json")) as _f:
    FIXTURE = json.load(_f)

# the frozen fp32 CelebA_DCRN_G64 forward at B = 8: 28 library calls
FROZEN_G64 = {"groupnorm_apply_parts_shortcut_f32": 3, "groupnorm_affine_parts_f32": 5, "groupnorm_act_f32": 1, "conv2d_fwd_x3_f32": 8,
              "conv2d_fwd_f32": 3, "fold_channels4_f32": 8}
# what the other routes of the layer run
ENTRIES = ["cslgan_" + n for n in (
    "groupnorm_act_bf16s", "conv2d_fwd_bf16s", "batchnorm_act_f32", "batchnorm_eval_act_f32", "norm_act_bwd_f32", "depth_to_space_f32",
    "groupnorm_apply_parts_f32", "cast_f32_bf16")]


@pytest.fixture
def harness(monkeypatch):
    return call_log.ModelHarness(monkeypatch.setattr)


def test_fixture_covers_every_case():
    assert set(FIXTURE) == set(call_log.CASES)
    assert len(FIXTURE) >= 30


def test_every_entry_is_reached():
    reached = {e for rec in FIXTURE.values() for e in rec["entries"]}
    wanted = set(ENTRIES) | {"cslgan_" + n for n in FROZEN_G64}
    assert not wanted - reached
    assert wanted <= set(call_log.ENTRIES)
    frozen = FIXTURE["g64_frozen_fp32"]["entries"]
    assert {e: frozen.count("cslgan_" + e) for e in FROZEN_G64} == FROZEN_G64 and len(frozen) == sum(FROZEN_G64.values())
    assert "cslgan_cast_f32_bf16" in FIXTURE["g64_frozen_recorder_bf16s"]["entries"]        # forward_shuffled's cast_bf16 arm


def _groups():
    """Case names by their first word (g64, g64bn, d64, nchw, ...): one test per group."""
    groups = {}
    for name in call_log.CASES:
        groups.setdefault(name.split("_")[0], []).append(name)
    return groups


@pytest.mark.parametrize("group", sorted(_groups()))
def test_call_logs(harness, group):
    """For every case the log equals the recorded one; a mismatch prints the current entries (the script's --case prints the full log)."""
    bad = []
    for name in _groups()[group]:
        log = harness.log(name)
        if call_log.lib_entries(log) != FIXTURE[name]["entries"]:
            bad.append("%s: recorded entries\n  %s\ncurrent entries\n  %s" % (name, FIXTURE[name]["entries"], call_log.lib_entries(log)))
        elif call_log.digest(log) != FIXTURE[name]["sha1"]:
            bad.append("%s: the same entries, another digest — compare `scripts/model_call_log.py --case %s` with the same command "
                       "under --root <the recorded commit>" % (name, name))
    assert not bad, "\n\n".join(bad)
