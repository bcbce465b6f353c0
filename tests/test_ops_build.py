"""The ops build and its sources: what the staleness check watches, what a
missing source does, that kernels are declared in one header only, and that
the extension's Python surface is the frozen one. No GPU needed."""

import os
import re
import subprocess

import pytest

from distributed_reinforcement_learning_amd import ops
from distributed_reinforcement_learning_amd.ops import build as ops_build

HIP_DIR = ops_build.HIP_DIR

# the names the PYBIND11_MODULE block defined before kernel declarations and
# launch constants moved into shared headers; that move must not show here
FROZEN_EXT_NAMES = {
    "normalize_frames_f32", "normalize_frames_bf16", "vtrace_scan",
    "vtrace_loss_fwd", "vtrace_loss_bwd", "mfma_probe", "conv_fwd",
    "conv_wgrad", "conv_dgrad", "relu_mask_bwd", "dqn_loss_fwd",
    "dqn_loss_bwd", "a2c_loss_fwd", "a2c_loss_bwd", "r2d2_loss_fwd",
    "dhead_train_fwd", "dhead_train_bwd", "dueling_head_fwd",
    "r2d2_loss_bwd", "per_update", "per_sample", "multi_gather",
    "per_rebuild", "embed_bwd", "lstm_tail_fwd", "lstm_tail_bwd",
    "mlp_heads_fwd", "mlp_heads_bwd", "embed_mlp_fwd", "embed_mlp_bwd",
    "mlp_heads_pack_wt", "mlp_heads_wgrad", "lstm_seq_train_fwd",
    "lstm_seq_train_bwd", "lstm_seq_fwd", "sq_norm", "grad_gather",
    "rmsprop_step", "rmsprop_step_t", "adam_step", "adam_step_t",
    "sq_norm_bf16", "rmsprop_step_bf16_t", "adam_step_bf16_t",
}


def _hip_files(suffix):
    return sorted(f for f in os.listdir(HIP_DIR) if f.endswith(suffix))


def _read(name):
    with open(os.path.join(HIP_DIR, name), encoding="utf-8") as f:
        return f.read()


def test_dependency_list_covers_every_file_in_the_so():
    deps = {os.path.relpath(p, HIP_DIR) for p in ops_build.dependency_paths()}
    assert "bind.cpp" in deps
    assert {"drla_common.h", "drla_kernels.h"} <= deps
    assert set(_hip_files(".hip")) <= deps
    assert set(_hip_files(".h")) <= deps
    for p in ops_build.dependency_paths():
        assert os.path.isfile(p), p


def test_missing_source_is_an_error_before_the_compiler_runs(monkeypatch):
    def no_compiler(*a, **k):
        raise AssertionError("compiler invoked despite a missing source")

    monkeypatch.setattr(ops_build, "SOURCES",
                        ops_build.SOURCES + ["no_such_kernel.hip"])
    monkeypatch.setattr(subprocess, "run", no_compiler)
    with pytest.raises(FileNotFoundError, match="no_such_kernel.hip"):
        ops_build.build(verbose=False, force=True)
    with pytest.raises(FileNotFoundError, match="no_such_kernel.hip"):
        ops_build.build(verbose=False, force=False)


def test_kernels_are_declared_in_one_header_only():
    hip = _hip_files(".hip")
    assert sorted(s for s in ops_build.SOURCES if s.endswith(".hip")) == hip
    for name in hip:
        assert re.search(r'^#include "drla_kernels\.h"$', _read(name),
                         re.M), f"{name} does not include drla_kernels.h"
    assert "__global__" not in _read("bind.cpp")
    assert '#include "drla_kernels.h"' in _read("bind.cpp")
    # every kernel a .hip file defines has its declaration in the header
    declared = set(re.findall(r"\b(drla_\w+)\(", _read("drla_kernels.h")))
    for name in hip:
        defined = set(re.findall(
            r'__global__[^;{(]*?\b(drla_\w+)\s*\(', _read(name)))
        defined |= set(re.findall(r"^CONV_KERNEL (drla_\w+)\(", _read(name),
                                  re.M))
        assert defined, name
        assert defined <= declared, (name, defined - declared)


def test_extension_names_are_the_frozen_set():
    if not ops.available():
        pytest.skip("extension not built")
    ext = ops.require_ext()
    public = {n for n in dir(ext) if not n.startswith("_")}
    assert public == FROZEN_EXT_NAMES
