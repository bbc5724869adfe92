"""CPU: the stage-2 and stage-3 trainers' memory layout -- `dvt_s2_workspace_bytes`, `dvt_s2_param_offsets`,
`dvt_s3_workspace_bytes{,_pos,_mp}`, `dvt_s3_param_offsets{,_pos}` -- equals, value for value, what the library answered
before the two steps shared one block and one carve (tests/golden/train_layout_parent.json, written by
tools/record_train_layout.py, which holds the table of configurations and the child process that asks)."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def recorder():
    spec = importlib.util.spec_from_file_location("record_train_layout", os.path.join(ROOT, "tools", "record_train_layout.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_layout_equals_the_parents(built_lib):
    from dvt_amd import _lib
    with open(os.path.join(ROOT, "tests", "golden", "train_layout_parent.json")) as f:
        want = json.load(f)["values"]
    got = recorder().layout(_lib.LIB_PATH)
    assert sorted(got) == sorted(want)
    assert len(want) == 36 * 5 + 12 * 21 and all(v >= 0 for v in want.values() if isinstance(v, int))
    wrong = [k for k in want if got[k] != want[k]]
    assert not wrong, f"{len(wrong)} of {len(want)} differ, first: {wrong[:5]}"
