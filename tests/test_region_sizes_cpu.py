"""The arena, scratch and workspace sizes of the fused-region units are part of what a caller allocates by: every *_save_bytes / *_scratch_bytes /
*_workspace_bytes query of csrc/regions.hip, fusion_head.hip and pool_head.hip returns exactly what tests/golden/region_sizes.json recorded
(tests/golden/region_sizes_record.py, run on the library of the commit before the arena carver and the nested Save layouts were shared).  No device is needed:
without one the split policies count on 256 compute units, the MI355X's."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _recorder():
    spec = importlib.util.spec_from_file_location("region_sizes_record", os.path.join(GOLDEN, "region_sizes_record.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()
with open(os.path.join(GOLDEN, "region_sizes.json")) as _f:
    TABLE = json.load(_f)


def test_the_table_holds_every_case_of_the_recorder():
    assert [(r["fn"], r["args"]) for r in TABLE] == [(fn, args) for fn, args in REC.cases()]
    fns = {r["fn"] for r in TABLE}
    for unit in ("encoder_block", "agg_block"):
        assert {f"devias_{unit}_{q}_bytes" for q in ("save", "scratch", "workspace")} <= fns
    assert {"devias_encoder_block_infer_workspace_bytes", "devias_head_save_bytes", "devias_head_workspace_bytes", "devias_fusion_head_save_bytes",
            "devias_fusion_head_workspace_bytes", "devias_pool_head_save_bytes", "devias_pool_head_workspace_bytes", "devias_softmax_ce_workspace_bytes", "devias_two_token_head_save_bytes",
            "devias_two_token_head_workspace_bytes", "devias_distill_workspace_bytes"} <= fns


def test_an_unsupported_row_dimension_sizes_to_zero():
    heads = [r for r in TABLE if r["fn"].startswith(("devias_fusion_head_", "devias_pool_head_", "devias_two_token_head_"))]
    bad = [r for r in heads if 512 in r["args"][:-1]]
    assert {r["fn"] for r in bad} == {r["fn"] for r in heads} and all(r["bytes"] == 0 for r in bad)
    assert all(r["bytes"] > 0 for r in TABLE if r not in bad)


@pytest.mark.parametrize("fn", sorted({r["fn"] for r in TABLE}))
def test_size_query_returns_the_recorded_bytes(fn):
    from devias_amd import _lib
    lib = _lib.load()
    for r in TABLE:
        if r["fn"] == fn:
            assert REC.query(lib, _lib, fn, r["args"]) == r["bytes"], (fn, r["args"])
