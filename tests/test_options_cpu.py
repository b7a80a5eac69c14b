"""The process-wide options (one table: csrc/common.h, values in csrc/api.hip) through the C ABI and devias_amd.ops, without a GPU: names, environment variables
and defaults are pinned here once; set / get, the reserve's clamp and policy, the error paths, the header's documentation and the ops.options scope."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

from devias_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (environment variable, default)
TABLE = {
    "gemm_epi": ("DEVIAS_GEMM_EPI", 1), "gemm256": ("DEVIAS_GEMM256", 1), "gemm_ss": ("DEVIAS_GEMM_SS", -1), "gemm_groupm": ("DEVIAS_GEMM_GROUPM", 0),
    "gemm_persistent": ("DEVIAS_GEMM_PERSIST", 1), "gemm_debug": ("DEVIAS_GEMM_DEBUG", 0), "gemm_epi_spec": ("DEVIAS_GEMM_EPI_SPEC", 1),
    "gemm_wt": ("DEVIAS_GEMM_WT", 1), "gemm_aux_nt": ("DEVIAS_GEMM_AUX_NT", 5), "gemm_smallm": ("DEVIAS_GEMM_SMALLM", 1),
    "gemm_tail_split": ("DEVIAS_GEMM_TAIL_SPLIT", 3), "gemm_w4": ("DEVIAS_GEMM_W4", -1), "gemm_splitk_xcd": ("DEVIAS_GEMM_SPLITK_XCD", 1),
    "gemm_dynamic": ("DEVIAS_GEMM_DYNAMIC", -1), "gemm_concurrent": ("DEVIAS_GEMM_CONCURRENT", 0), "gemm_reserve_cus": ("DEVIAS_GEMM_RESERVE_CUS", 0),
    "attn_cfg": ("DEVIAS_ATTN_CFG", 0), "attn_xcd": ("DEVIAS_ATTN_XCD", 1), "attn_bias_fused": ("DEVIAS_ATTN_BIAS_FUSED", 1),
    "attn_dkdv": ("DEVIAS_ATTN_DKDV", 1), "attn_qpre": ("DEVIAS_ATTN_QPRE", 1), "regions_defer": ("DEVIAS_REGIONS_DEFER", 1),
    "slot_mfma": ("DEVIAS_SLOT_MFMA", 1),
}


def _child_options(env_changes):
    """[(name, value), ...] of every option as a fresh process sees them, started without any DEVIAS_* variable but `env_changes`"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("DEVIAS_")}
    env.update(env_changes)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    code = "import json; from devias_amd import ops; print(json.dumps([(n, ops.get_option(n)) for n in ops.option_names()]))"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return [tuple(x) for x in json.loads(r.stdout.strip().splitlines()[-1])]


def test_defaults_without_environment():
    got = _child_options({})
    names = [n for n, _ in got]
    assert len(names) == 23 and len(set(names)) == 23
    assert dict(got) == {n: d for n, (_, d) in TABLE.items()}


def test_every_option_reads_its_environment_variable():
    want = {n: 101 + i for i, n in enumerate(TABLE)}
    got = _child_options({TABLE[n][0]: str(v) for n, v in want.items()})
    assert dict(got) == want


def test_set_get_round_trip_reserve_policy_and_error_paths():
    lib = _lib.load()
    assert set(ops.option_names()) == set(TABLE)
    assert lib.devias_option_name(-1) is None and lib.devias_option_name(len(TABLE)) is None
    with ops.options():
        for i, n in enumerate(ops.option_names()):
            ops.set_option(n, 7 + i)
            assert ops.get_option(n) == 7 + i
        ops.set_option("gemm_reserve_cus", -5)
        assert ops.get_option("gemm_reserve_cus") == 0
        info = (ctypes.c_int64 * 5)()
        cus = int(info[0]) if lib.devias_device_info(0, info) == 0 else 256        # (no device: the library counts on 256 CUs)
        for r in (0, 8, 13, 64, 100000):
            ops.set_option("gemm_reserve_cus", r)
            assert lib.devias_policy_gemm_cus() == max(cus - r, 8) & ~7, r
    v = ctypes.c_int32(0)
    for name in (b"no_such_option", b"x" * 4000):
        assert lib.devias_set_option(name, 1) == -1
        msg = lib.devias_last_error()
        assert msg.startswith(b"devias_set_option: unknown option '" + name[:64]) and len(msg) < 512
        assert lib.devias_get_option(name, ctypes.byref(v)) == -1
        msg = lib.devias_last_error()
        assert msg.startswith(b"devias_get_option: unknown option '" + name[:64]) and len(msg) < 512
    assert lib.devias_set_option(None, 1) == -1 and lib.devias_last_error() == b"devias_set_option: null name"
    assert lib.devias_get_option(None, ctypes.byref(v)) == -1 and lib.devias_last_error() == b"devias_get_option: null argument"
    assert lib.devias_get_option(b"gemm_epi", None) == -1 and lib.devias_last_error() == b"devias_get_option: null argument"
    with pytest.raises(RuntimeError, match="unknown option 'no_such_option'"):
        ops.set_option("no_such_option", 1)


def test_header_documents_exactly_the_options():
    hdr = open(os.path.join(ROOT, "include", "devias_amd.h")).read()
    block = hdr[hdr.index("/* Process-wide integer options"):hdr.index("int devias_set_option(")]
    assert set(re.findall(r'"(\w+)"', block)) == set(ops.option_names())
    # one entry per option, in table order, with its variable and default
    entries = re.findall(r'^ \*   "(\w+)"\s+(DEVIAS_\w+)\s+(-?\d+)\s', block, flags=re.M)
    assert [(n, (e, int(d))) for n, e, d in entries] == [(n, TABLE[n]) for n in ops.option_names()]


def test_options_scope_restores_nests_and_rejects_unknown_names():
    before = {n: ops.get_option(n) for n in ops.option_names()}

    def now():
        return {n: ops.get_option(n) for n in ops.option_names()}
    with pytest.raises(KeyError):                                  # an exception inside the block
        with ops.options(gemm_smallm=0, attn_dkdv=2):
            assert ops.get_option("gemm_smallm") == 0 and ops.get_option("attn_dkdv") == 2
            raise KeyError("x")
    assert now() == before
    with ops.options():                                            # a plain set_option inside the block
        ops.set_option("gemm_w4", 15)
        ops.set_option("slot_mfma", 0)
    assert now() == before
    with ops.options(gemm_tail_split=0):                           # nested scopes
        with ops.options(gemm_tail_split=4, gemm_epi=0):
            assert (ops.get_option("gemm_tail_split"), ops.get_option("gemm_epi")) == (4, 0)
        assert (ops.get_option("gemm_tail_split"), ops.get_option("gemm_epi")) == (0, before["gemm_epi"])
    assert now() == before
    with pytest.raises(ValueError, match="no_such_option"):        # nothing is changed when a name is unknown
        with ops.options(gemm_smallm=0, no_such_option=1):
            pytest.fail("the block must not run")
    assert now() == before
