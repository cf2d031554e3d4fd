"""The run plan (csrc/run_plan.h) on the host alone: the header holds no HIP type, so run_plan_walk.cpp compiles it with
the host compiler under the address and undefined-behaviour sanitizers and prints every field of the plan of a shape
under given knob values.  Each plan must equal np_run_plan.plan -- the gates restated from build_kparams and the host
launchers as they stood before the header existed -- and hold the properties np_run_plan.check_properties names.  The
library's own answers (acmmp_strip_plan, acmmp_keep_mask_bytes) must agree with the plan too.  No GPU."""
import itertools
import os
import subprocess

import pytest

import np_run_plan as rp
from acmmp import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (model, W, H, patch_size, radius_increment)
SHAPES = [(11, 2000, 1000, 11, 2), (11, 1998, 1000, 11, 2), (11, 2000, 998, 11, 2), (11, 4000, 2000, 21, 4),
          (11, 2000, 1000, 7, 2), (0, 640, 480, 11, 2),
          (11, 8192, 4096, 11, 2),                     # a colour grid of 2^24 pixels: no fallback queue
          (11, 32768, 32768, 11, 2)]                   # 2^29: no split either (arithmetic only, nothing is allocated)
VIEWS = [1, 2, 4, 5, 8, 9, 15, 31]
# every knob at its default, then flipped once
FLIPS = [{}, {"ACMMP_INTERP": "0"}, {"ACMMP_PIN_HOMOG": "0"}, {"ACMMP_SPREAD_MAX": "8"}, {"ACMMP_NEG_TAU": "0.125"},
         {"ACMMP_NEG_SKIP": "0"}, {"ACMMP_REF_NEG_TAU": "0.125"}, {"ACMMP_REF_NEG_SKIP": "0"}, {"ACMMP_KEEP_MASK": "0"},
         {"ACMMP_NBFIX_MAX_PC": "1000"}, {"ACMMP_DEAD_SKIP": "0"}, {"ACMMP_REF_SPLIT": "0"}, {"ACMMP_REF_SPLIT_AT": "3"},
         {"ACMMP_REF_SPLIT_AT": "12"}, {"ACMMP_NB_VIEW_CHUNK": "4"}, {"ACMMP_NB_VIEW_CHUNK": "0"}, {"ACMMP_NB_TILE": "0"},
         {"ACMMP_STRIPS": "2"}, {"ACMMP_STRIPS": "4"}, {"ACMMP_STRIP_STREAMS": "2"}, {"ACMMP_KERNEL_TIMING": "all"},
         {"ACMMP_KERNEL_TIMING": "1"}]
WANT = [0, 1, 2, 4, 64]
FLOATS = ("spread_max", "neg_tau", "ref_neg_tau")
LISTS = ("bounds", "ref_blocks", "fix_cap")


def cases():
    for (model, W, H, ps, inc), V, fast, tex16, geom in itertools.product(SHAPES, VIEWS, (1, 0), (1, 0), (0, 1)):
        shape = dict(model=model, W=W, H=H, V=V, patch_size=ps, radius_increment=inc, fast=fast, tex16=tex16, geom=geom,
                     want_strips=0)
        for env in FLIPS:
            yield shape, env
        for want in WANT[1:]:
            yield dict(shape, want_strips=want), {}
    for ps, inc in [(131, 2), (17, 1)]:                # radius > 64; more than 64 samples
        yield dict(model=11, W=2000, H=1000, V=2, patch_size=ps, radius_increment=inc, fast=1, tex16=1, geom=0,
                   want_strips=0), {}


def parse(block):
    p = {}
    for line in block.splitlines():
        name, *vals = line.split()
        if name == "error":
            p[name] = " ".join(vals)
        elif name in LISTS:
            p[name] = [int(v) for v in vals]
        elif name in FLOATS:
            p[name] = float.fromhex(vals[0])
        else:
            p[name] = int(vals[0])
    return p


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("walk") / "run_plan_walk")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "acmmp-spherical_amd", "csrc"),
                    os.path.join(ROOT, "tests", "run_plan_walk.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def plans(walk):
    """[(shape, env, the header's plan)] of the whole matrix, from one process."""
    todo = list(cases())
    text = "".join(" ".join(f"{k}={v}" for k, v in {**shape, **env}.items()) + "\n" for shape, env in todo)
    out = subprocess.run([walk, "-"], input=text, check=True, capture_output=True, text=True)
    assert out.stderr == ""
    blocks = out.stdout.split("end\n")
    assert blocks[-1] == "" and len(blocks) == len(todo) + 1
    return [(shape, env, parse(b)) for (shape, env), b in zip(todo, blocks)]


def test_one_case_on_the_command_line(walk):
    shape = dict(model=11, W=2000, H=1000, V=2, patch_size=11, radius_increment=2, fast=1, tex16=1, geom=0, want_strips=0)
    env = {"ACMMP_STRIPS": "4", "ACMMP_NEG_TAU": "0.125"}
    out = subprocess.run([walk] + [f"{k}={v}" for k, v in {**shape, **env}.items()], check=True, capture_output=True,
                         text=True)
    assert out.stderr == ""
    assert parse(out.stdout) == rp.plan(shape, env)


@pytest.mark.parametrize("flip", range(len(FLIPS)), ids=["-".join(f"{k[6:]}={v}" for k, v in f.items()) or "defaults"
                                                       for f in FLIPS])
def test_plan_equals_the_restatement(plans, flip):
    n = 0
    for shape, env, got in plans:
        if env == FLIPS[flip] and (flip > 0 or shape["want_strips"] == 0):
            assert got == rp.plan(shape, env), (shape, env)
            n += 1
    assert n >= len(SHAPES) * len(VIEWS) * 8


def test_wanted_strips(plans):
    for shape, env, got in plans:
        if shape["want_strips"] > 0:
            assert got == rp.plan(shape, env), shape
            assert got["ns"] <= shape["want_strips"]


def test_unsupported_shapes(plans):
    bad = [(got["status"], got["error"]) for shape, env, got in plans if got["status"]]
    assert bad == [(1, "patch radius > 64"), (2, "more than 64 patch samples (patch_size / radius_increment)")]


def test_properties(plans):
    seen = set()
    for shape, env, got in plans:
        rp.check_properties(got, shape)
        if not got["status"]:
            seen |= {("keep", got["keep"]), ("queue", got["fix_queue"]), ("ref_fix", got["ref_fix"]), ("ns", got["ns"]),
                     ("init", got["init_inst"]), ("ref", got["ref_inst"]), ("masked", got["nb_masked"]),
                     ("split", got["ref_split"] > 0), ("interp", got["interp"], got["ref_interp"])}
    # the matrix reaches every branch of the plan
    assert seen >= {("keep", 0), ("keep", 1), ("queue", 0), ("queue", 1), ("ref_fix", 0), ("ref_fix", 1), ("ns", 1),
                    ("ns", 2), ("ns", 4), ("init", 0), ("init", 1), ("init", 3), ("ref", 0), ("ref", 1), ("ref", 2),
                    ("masked", 0), ("masked", 1), ("split", False), ("split", True), ("interp", 0, 0), ("interp", 1, 0),
                    ("interp", 1, 1)}


def test_large_grids_have_no_queue_and_no_split(plans):
    for shape, env, got in plans:
        if shape["W"] >= 8192 and shape["fast"] and shape["tex16"]:
            assert not got["fix_queue"] and not got["interp"] and got["neg_tau"] < 0 and got["nbfix_n"] == 0
        if shape["W"] == 32768:
            assert got["ref_split"] == 0 and got["Pc"] == 1 << 29


def test_strip_bounds_equal_the_librarys(plans):
    for shape, env, got in plans:
        if not got["status"] and (shape["want_strips"] > 0 or "ACMMP_STRIPS" in env):
            want = shape["want_strips"] or int(env["ACMMP_STRIPS"])
            bounds, _ = capi.strip_plan(got["rows"], want if got["ns"] > 1 else got["ns"])
            assert bounds == got["bounds"], (shape, env)


SLAB_KNOBS = ("ACMMP_KEEP_MASK", "ACMMP_REF_NEG_SKIP", "ACMMP_REF_NEG_TAU")
# the rows of tests/test_keep_mask_slab.py: keep_mask_bytes' arguments and the environment
SLAB_ROWS = [(dict(W=2000, H=1000, n_src=2), {}), (dict(W=2000, H=1500, n_src=4), {}), (dict(W=2001, H=1001, n_src=1), {}),
             (dict(W=4000, H=2000, n_src=3), {}), (dict(W=2000, H=1000, n_src=4), {}), (dict(W=2000, H=1000, n_src=5), {}),
             (dict(W=2000, H=1000, fast=False), {}), (dict(W=2000, H=1000, tex16=False), {}),
             (dict(W=2000, H=1000, model=0), {}), (dict(W=2000, H=1000, geom=True), {}), (dict(W=1998, H=1000), {}),
             (dict(W=2000, H=998), {}), (dict(W=2000, H=1000, patch_size=7), {}),
             (dict(W=4000, H=2000, patch_size=21, radius_increment=4), {}),
             (dict(W=2000, H=1000), {"ACMMP_KEEP_MASK": "0"}),
             (dict(W=2000, H=1000), {"ACMMP_KEEP_MASK": "1", "ACMMP_REF_NEG_SKIP": "0"}),
             (dict(W=2000, H=1000), {"ACMMP_KEEP_MASK": "1", "ACMMP_REF_NEG_TAU": "0.125"})]


@pytest.mark.parametrize("row", range(len(SLAB_ROWS)))
def test_keep_mask_bytes_of_the_library_equal_the_plans(walk, monkeypatch, row):
    args, env = SLAB_ROWS[row]
    for k in SLAB_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a = dict(dict(model=11, patch_size=11, radius_increment=2, fast=True, tex16=True, n_src=4, geom=False), **args)
    shape = dict(model=a["model"], W=a["W"], H=a["H"], V=a["n_src"], patch_size=a["patch_size"],
                 radius_increment=a["radius_increment"], fast=int(a["fast"]), tex16=int(a["tex16"]), geom=int(a["geom"]),
                 want_strips=0)
    out = subprocess.run([walk] + [f"{k}={v}" for k, v in {**shape, **env}.items()], check=True, capture_output=True,
                         text=True)
    assert capi.keep_mask_bytes(**args) == parse(out.stdout)["keep_mask_bytes"] == rp.plan(shape, env)["keep_mask_bytes"]
