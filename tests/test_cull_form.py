"""Which kernel a cluster pass launches (niagara_amd/csrc/cullform.h choose_cull_form) on the CPU: the header the library compiles is built HERE with g++
(tests/cullform_shim.cpp) and held, row by row, to a decision table recorded from the code BEFORE the choice became one function.

tests/golden/cull_form_table.npz — how it was made: a throw-away g++ program held the statements of that earlier commit verbatim (nv_clustercull's and
nv_taskcull's hint / option / provenance logic, launch_cluster_mask's and launch_cc's if-trees with the kernel launches replaced by a note of the template
arguments, count_cull_variant, clustercull_takes_packed, the three clustercull_prefers_* rules) over stand-in context / argument structs, enumerated the
inputs below and wrote what those statements launched and counted.  295 488 rows: every combination of
    entry x late (nv_clustercull early / late, nv_taskcull's early pass) x clusterOcclusionEnabled x postPass x SoA mirror x filterK > 0
    x NV_OPT_CULL_FORM 0-5 x NV_OPT_CULL_RING 0 / 4 / 8 x own task list or not
with each of 77 hint-word scenarios (no words; command count 0 / 1 / CC_SHALLOW_COMMANDS / + 1 / 250 000 x filter statistic 0 % / just below / just above
directPercent / 100 %; the task pass's (commands, emitting draws) at fill 59 / 60 / 61 / 84 / 85 / 86 % and with either word 0; nv_taskcull's own count
word) and, for the scenarios that can feel them, mirroredCount on both sides of the 48 MiB rule, the always-deep bit and an explicit command count.  The
same program compared the new function with the old statements over the FULL cartesian grid of these values (24.9 M rows, also at directPercent 50) before the
table was cut down to a committable size: no difference.

NV_VARIANT_CULL_LANES never appears: no launch has counted it since 0.4 (include/niagara_vis.h), before and after, so the table cannot hold it; the test
pins that instead."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = ["entry", "late", "clusterOcclusionEnabled", "postPass", "soa", "filterPositive", "cull_form", "cull_ring", "directPercent", "hints", "hint0", "hint1", "hint2",
          "hint3", "hint4", "ownTaskCommands", "mirroredCount", "alwaysDeep", "commandCountOverride"]
OUTPUTS = ["family", "late", "soa", "bits", "depth", "direct", "defer", "pack", "twoStage", "deferHiz", "packDirect", "packBits", "expectedCmds", "packedTable", "variant"]
FORM_COLUMNS = [c for c in OUTPUTS if c != "expectedCmds"]  # the table's `forms` rows
FLAG_COLUMNS = ["entry", "late", "clusterOcclusionEnabled", "postPass", "soa", "filterPositive", "cull_form", "cull_ring", "directPercent", "ownTaskCommands", "alwaysDeep"]

# <LATE, SOA, BITS, ring depth, DIRECT, DEFER, PACK> of every cluster_mask_kernel the launcher could be made to launch before this table was recorded: launch_cc<LATE, SOA,
# DEPTH, DIRECT> for the seven (LATE, SOA, DEPTH, DIRECT) launch_cluster_mask named, each by deferHiz / visibility bits / packDirect / packBits
T, F = 1, 0
MASK_FORMS = {
    (F, T, F, 8, T, T, F), (T, T, F, 8, T, F, F), (F, T, F, 8, T, T, T), (F, T, T, 8, T, F, T), (F, T, T, 8, T, F, F), (F, T, F, 8, T, F, T), (F, T, F, 8, T, F, F),
    (F, T, F, 8, F, T, F), (T, T, F, 8, F, F, F), (F, F, F, 8, F, T, F), (T, F, F, 8, F, F, F),
    (F, T, F, 4, F, T, F), (F, T, T, 4, F, F, F), (F, T, F, 4, F, F, F), (F, T, T, 8, F, F, F), (F, T, F, 8, F, F, F), (F, F, T, 8, F, F, F), (F, F, F, 8, F, F, F),
}
# instantiated, but out of the entry points' reach since the late pass with visibility bits became two-stage (it launches the early form): LATE with BITS
MASK_FORMS_NEVER_CHOSEN = {(T, T, T, 8, T, F, F), (T, T, T, 8, F, F, F), (T, F, T, 8, F, F, F)}
BITS_FORMS = {(T,), (F,)}  # cluster_bits_kernel<SOA, true>

VARIANT = {"cull_filter_ring4": 0, "cull_filter_ring8": 1, "cull_direct": 2, "cull_lanes_bits": 3, "cull_lanes": 4, "cull_aos": 5, "cull_direct_packed": 9}


@pytest.fixture(scope="module")
def table():
    z = np.load(os.path.join(ROOT, "tests", "golden", "cull_form_table.npz"))
    n = z["hint_row"].shape[0]
    ins = np.zeros((n, len(INPUTS)), np.uint32)
    for i, name in enumerate(FLAG_COLUMNS):
        ins[:, INPUTS.index(name)] = z["flags"][i]
    ins[:, INPUTS.index("hints"):INPUTS.index("hint4") + 1] = z["hint_words"][z["hint_row"]]
    ins[:, INPUTS.index("mirroredCount")] = z["mirrored_count"]
    ins[:, INPUTS.index("commandCountOverride")] = z["command_count_override"]
    outs = np.zeros((n, len(OUTPUTS)), np.uint32)
    outs[:, [OUTPUTS.index(c) for c in FORM_COLUMNS]] = z["forms"][z["answer_row"]]
    outs[:, OUTPUTS.index("expectedCmds")] = z["expected_cmds"]
    return ins, outs


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cullform") / "cullform_shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", os.path.join(ROOT, "tests", "cullform_shim.cpp"), "-o", so], check=True)
    return C.CDLL(so)


def col(a, names, name):
    return a[:, names.index(name)]


def test_choose_cull_form_answers_every_row_as_the_code_before_it_did(shim, table):
    ins, want = table
    got = np.zeros_like(want)
    shim.shim_choose_cull_form(np.ascontiguousarray(ins).ctypes.data_as(C.c_void_p), C.c_uint32(len(ins)), got.ctypes.data_as(C.c_void_p))
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "%d of %d rows differ; first: inputs %s\n want %s\n  got %s" % (
        bad.size, len(ins), dict(zip(INPUTS, ins[bad[0]].tolist())), dict(zip(OUTPUTS, want[bad[0]].tolist())), dict(zip(OUTPUTS, got[bad[0]].tolist())))


def test_the_table_is_not_vacuous(table):
    ins, outs = table
    mask = col(outs, OUTPUTS, "family") == 0
    params = [OUTPUTS.index(c) for c in ("late", "soa", "bits", "depth", "direct", "defer", "pack")]
    assert {tuple(r) for r in np.unique(outs[mask][:, params], axis=0).tolist()} == MASK_FORMS  # every instantiation the launcher could launch, and no other
    assert {tuple(r) for r in np.unique(outs[~mask][:, [OUTPUTS.index("soa")]], axis=0).tolist()} == BITS_FORMS
    assert (col(outs, OUTPUTS, "bits")[~mask] == 1).all()
    # every NV_VARIANT_CULL_* slot a launch can count; cull_lanes has had no launch since 0.4 (module docstring)
    assert set(np.unique(col(outs, OUTPUTS, "variant")).tolist()) == {v for k, v in VARIANT.items() if k != "cull_lanes"}
    # the packed walk and its delay table go together, and the argument word says what the second stage needs
    assert (col(outs, OUTPUTS, "pack") == col(outs, OUTPUTS, "packedTable")).all() and (col(outs, OUTPUTS, "twoStage") == col(outs, OUTPUTS, "deferHiz")).all()
    # the task-payload entry is not the cluster entry: same inputs otherwise, another answer
    entry = col(ins, INPUTS, "entry")
    rest = [i for i, n in enumerate(INPUTS) if n != "entry"]
    early = (entry == 0) & (col(ins, INPUTS, "late") == 0)
    task = entry == 1
    assert early.sum() == task.sum() and (ins[early][:, rest] == ins[task][:, rest]).all()  # (the generator's loop order pairs them)
    differ = (outs[early] != outs[task]).any(axis=1)
    assert differ.any() and not differ.all()
    # both sides of every threshold are in the inputs
    assert {0, 1, 500000, 500001, 250000} <= set(np.unique(col(ins, INPUTS, "hint0")).tolist())
    assert set(np.unique(col(ins, INPUTS, "cull_form")).tolist()) == set(range(6)) and set(np.unique(col(ins, INPUTS, "cull_ring")).tolist()) == {0, 4, 8}
    assert set(np.unique(col(ins, INPUTS, "mirroredCount")).tolist()) == {(48 << 20) // 12, (48 << 20) // 12 + 1}


def test_the_launcher_has_one_case_per_form_and_the_names_are_the_bindings():
    """launch_cluster_mask's dispatch (clustercull.hip) lists exactly the instantiations above, and the variant slots the table counts are the names
    pipeline.Context.VARIANTS gives them (bench.py and tools/ read them by name)"""
    src = open(os.path.join(ROOT, "niagara_amd", "csrc", "clustercull.hip")).read()
    cases = re.findall(r"^\s*CC_CASE\(([^)]*)\)", src, re.M)
    forms = [tuple({"true": 1, "false": 0}.get(w.strip(), w.strip()) for w in c.split(",")) for c in cases]
    forms = [tuple(int(w) for w in f) for f in forms]
    assert len(forms) == len(set(forms)) and set(forms) == MASK_FORMS | MASK_FORMS_NEVER_CHOSEN
    header = open(os.path.join(ROOT, "include", "niagara_vis.h")).read()
    slots = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define NV_VARIANT_(\w+) (\d+)", header) if m.group(1) != "SLOTS"}
    names = re.search(r"VARIANT_NAMES = \(([^)]*)\)", open(os.path.join(ROOT, "niagara_amd", "_lib.py")).read()).group(1)
    names = [w.strip().strip('"') for w in names.split(",") if w.strip()]
    assert {n: i for i, n in enumerate(names)} == slots and all(slots[k] == v for k, v in VARIANT.items())
