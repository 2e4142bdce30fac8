"""Tile groups of the S assembly (ba_kernels.h: sgroup_code) on the host-side packing, no GPU needed: every tile of the merged
Gram launch is in exactly one group, a group never crosses a workgroup window of G positions nor mixes tuples, and the compact
camera entry list keeps one entry per camera of every group."""
import numpy as np
import pytest

from tests import helpers as H


def _problem(name):
    if name == "band":
        return H.make(40, 2000, 4, seed=411)
    if name == "ragged":
        return H.make(120, 6000, 6, seed=412, dropout=0.35)
    if name == "mixed":          # tracks of 2..4 cameras: several operand heights in one merged launch
        return H.make(50, 3000, 3, seed=413, dropout=0.2)
    if name == "clustered":
        return H.make(60, 3000, 5, seed=414, mode="unordered")
    raise ValueError(name)


@pytest.mark.parametrize("name", ["band", "ragged", "mixed", "clustered"])
@pytest.mark.parametrize("G", [2, 4])
def test_sgroup_table(lib, name, G):
    from xrsfm_amd import capi
    g = capi.debug_sgroup(H.to_product(_problem(name)), G)
    n, tiles, codes = g["positions"], g["pos_tile"], g["pos_code"]
    ncam = g["gram"]["tile_ncam"]
    assert n == int(((ncam > 0) & (ncam <= 8)).sum()) or n == g["gram"]["items_small"]
    assert len(set(tiles.tolist())) == n                       # every tile of the launch once
    idx, ln = codes & 15, codes >> 4
    q = 0
    dropped = 0
    while q < n:
        L = int(ln[q])
        assert idx[q] == 0 and 1 <= L <= G
        assert q // G == (q + L - 1) // G                      # inside one workgroup window
        run = tiles[q:q + L]
        for j in range(L):
            assert idx[q + j] == j and ln[q + j] == L
        if L > 1:
            t0 = run[0]
            Ls = g["tile_stride"][t0]
            assert 2 <= Ls <= 4 and ncam[t0] == Ls
            for t in run[1:]:                                  # one tuple, same cidx order
                assert g["tile_stride"][t] == Ls and ncam[t] == Ls
                assert np.array_equal(g["tile_cams"][t], g["tile_cams"][t0])
                assert np.array_equal(g["tile_cidx"][t], g["tile_cidx"][t0])
            dropped += (L - 1) * int(Ls)
        q += L
    assert g["cam_entries_kept"] == g["cam_entries"] - dropped   # one entry per camera of each group
    cp = g["cam_ptr_s"]
    assert cp[0] == 0 and cp[-1] == g["cam_entries_kept"] and np.all(np.diff(cp) >= 0)
    if name == "band":
        assert dropped > 0                                     # the banded map does group


def test_sgroup_one_is_no_grouping(lib):
    from xrsfm_amd import capi
    g = capi.debug_sgroup(H.to_product(_problem("band")), 1)
    assert np.all(g["pos_code"] == 16) and g["cam_entries_kept"] == g["cam_entries"]
