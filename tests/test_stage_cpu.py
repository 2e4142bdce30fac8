"""ba_stage.h alone, as a host program under the address and undefined-behaviour sanitizers (tests/stage_host_driver.py): the block
layout of the one-shot calls against the rule recomputed here, the view over the read-back buffer, the trial-bound rows and the
check of an offsets array.  No GPU."""
import pytest

from tests import stage_host_driver as H

I, O, E = "I", "O", "E"


def rule(tokens):
    """cumulative (max(b, 8) + 255) & ~255 -> (offsets, (in_bytes, out0, out_bytes, total), output offsets relative to out0)"""
    off, offs, outs, in_out = 0, [], [], False
    in_bytes = out0 = out_bytes = 0
    for t in tokens:
        if t == I:
            in_bytes = off
        elif t == O:
            out0, in_out = off, True
        elif t == E:
            out_bytes, in_out = off - out0, False
        else:
            offs.append(off)
            if in_out:
                outs.append(off - out0)
            off += (max(int(t), 8) + 255) & ~255
    return offs, (in_bytes, out0, out_bytes, off), outs


# the five one-shot layouts at their smallest counts, array by array as the entries take them
# (CamRec 128 B, PnpFrame 24 B, InitPair and FundPair 32 B; one trial, so 3 or 5 sample indices per item)
FILTER = [128 * 0, 4 * 0, 24 * 1, 4 * 2, 4 * 0, 16 * 0, I, 24 * 0, O, 8, 0, 1, 8, 8, E]                         # Nc 0, Np 1, No 0
TRIANGULATE = [128, 4 * 2, 4 * 2, 16 * 2, 4 * 129 * 129, I, 24, O, 24, 4, 4, 4, 1, 2, E, 32]                    # Nc 1, Nt 1, No 2
ABSOLUTE_POSE = [24, 16 * 3, 24 * 3, 4 * 3, 4 * 4, I, O, 32, 24, 4, 4, 4, 1, 3, E]                              # Nf 1, Nc 3
TWO_VIEW = [32, 32 * 10, 4 * 5, 4 * 11, I, O, 72, 32, 24, 24 * 10, 32, 4, 4, 1, 1, 10, 10, E, 8 * 9 * 10 * 64]  # Np 1, Nm 10
VERIFY = [32, 32 * 15, 4 * 16, I, O, 72, 4, 4, 4, 1, 15, E]                                                     # Np 1, Nm 15

CASES = {
    "all_zero": [0, 0, 0, I, 0, O, 0, 0, E, 0],
    "filter": FILTER, "triangulate": TRIANGULATE, "absolute_pose": ABSOLUTE_POSE, "two_view": TWO_VIEW, "verify": VERIFY,
    "device_only_between": [100, 7, I, 300, 1, O, 64, 9, E],
    "device_only_after": [100, I, O, 64, 9, E, 5000, 1],
    "around_256": [255, 256, 257, I, O, 257, 256, 255, E],
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return H.build(tmp_path_factory.mktemp("stage_rule"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_layout_is_the_cumulative_rule(driver, name):
    tokens = CASES[name]
    offs, marks, rel = H.parse_layout(H.run(driver, H.layout_input(tokens))[0])
    want_offs, want_marks, want_rel = rule(tokens)
    assert offs == want_offs
    assert marks == want_marks
    assert rel == want_rel                                  # the view finds every output where the read-back put it
    assert all(o % 256 == 0 for o in offs) and len(set(offs)) == len(offs)          # own slot, 256-aligned, empty arrays too
    in_bytes, out0, out_bytes, total = marks
    assert in_bytes <= out0 and out0 + out_bytes <= total and in_bytes % 256 == 0 and out_bytes % 256 == 0


def test_sizes_around_a_slot():
    offs, marks, _ = rule(CASES["around_256"])
    assert offs == [0, 256, 512, 1024, 1536, 1792] and marks == (1024, 1024, 1024, 2048)        # (the rule itself, spelt out once)


def test_trial_rows_are_shared_by_the_items_of_one_n(driver):
    ns = [5, 3, 5, 7, 3, 3]
    offs, rows = H.parse_rows(H.run(driver, H.rows_input(ns))[0])
    first, want_rows = {}, []
    for n in ns:
        if n not in first:
            first[n] = len(want_rows)
            want_rows += [1000 * n + i for i in range(n + 1)]           # a new n appends its row of n + 1 entries
    assert offs == [first[n] for n in ns]                                # two items of the same n share one offset
    assert rows == want_rows


@pytest.mark.parametrize("wide", (False, True))
def test_offsets_array_check(driver, wide):
    ask = lambda name, v: H.run(driver, H.offsets_input(name, v, wide))[0]
    assert ask("trk_ptr", [0, 2, 1]) == "trk_ptr decreases"
    assert ask("trk_ptr", [1, 2]) == "trk_ptr does not start at 0"
    assert ask("desc_ptr", [1, 0]) == "desc_ptr does not start at 0"      # (the start is looked at first)
    assert ask("match_ptr", [0]) == "ok"
    assert ask("match_ptr", [0, 0, 3, 3]) == "ok"
    if wide:
        assert ask("key_ptr", [0, 1 << 40, (1 << 40) - 1]) == "key_ptr decreases"
