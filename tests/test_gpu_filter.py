"""The post-BA track filter on the GPU (xrsfm_ba_filter_tracks: k_cam_centres and k_filter_tracks of ba_filter.h, filter_tracks_impl) against
the long-double yardstick of tests/filter_yardstick.py on the catalogue of tests/filter_cases.py: every case at every setting through
capi.filter_tracks, obs_delete, track_outlier and num_filtered bit for bit, track_error and track_angle of every track within its own bar
(-1.0 exactly where the rule leaves them unset, NaN where the rule gives NaN); every call repeated once, bit-identical; the permuted and the
relabelled scene give the ordered scene's outputs, permuted, bit for bit; the exact-threshold cases give the hand-written masks.

The limit is 1 bar everywhere.  Largest ratios |got - value| / bar per check and case group as MEASURED on an MI355X (measured values, not
limits; obs_delete, track_outlier and num_filtered are 0 = identical everywhere):

    group        track_error   track_angle
    generated    0.159         0.095
    lengths      0.084         0.030
    launch       0.248         0.137
    order        0.096         0.088
    exit         0.085         0.045
    degenerate   0.119         0.025
    exact        0.017         0.114
    near         0.106         0.085
    nonfinite    0.068         0.113
"""
import numpy as np
import pytest

from tests import filter_cases as FC
from tests import filter_yardstick as Y
from tests import helpers as H

pytestmark = pytest.mark.gpu

OUTPUTS = ("obs_delete", "track_outlier", "track_error", "track_angle", "num_filtered")


def run(name, k):
    from xrsfm_amd import capi
    return capi.filter_tracks(H.to_product(FC.case(name)), *FC.settings(name)[k])


def same_bits(a, b):
    return [key for key in OUTPUTS if np.ascontiguousarray(a[key]).tobytes() != np.ascontiguousarray(b[key]).tobytes()]


@pytest.mark.parametrize("name,k", FC.RUNS)
def test_every_decision_against_the_yardstick(lib, name, k):
    got, again = run(name, k), run(name, k)
    checks = Y.check(FC.reference(name, k), got)
    print("filter-ratio %-10s %-14s %d  %s" % (FC.group_of(name), name, k, "  ".join("%s %.4f" % kv for kv in Y.worst(checks).items())))
    assert Y.failures(checks) == {}
    assert same_bits(got, again) == []


@pytest.mark.parametrize("name", ("order_shuffled", "order_relabel"))
def test_the_callers_order_does_not_matter(lib, name):
    """the same observations in another order, the same tracks under other labels: the ordered scene's outputs, permuted, bit for bit"""
    base, got = run("order_base", 0), run(name, 0)
    obs_map, pt_map = FC.ORDER_MAPS[name]
    want = dict(obs_delete=base["obs_delete"][obs_map], track_outlier=base["track_outlier"][pt_map], track_error=base["track_error"][pt_map],
                track_angle=base["track_angle"][pt_map], num_filtered=base["num_filtered"])
    assert same_bits(got, want) == []
    assert base["obs_delete"].sum() > 20 and set(base["track_outlier"].tolist()) == {0, 1, 2}


def test_the_exact_thresholds_give_the_hand_written_masks(lib):
    for k, want in enumerate(FC.EXACT_EXPECT):
        got = run("exact", k)
        for key, value in want.items():
            assert got[key].tolist() == value, (k, key)
        assert got["track_error"][4] == (5.0 if k == 0 else -1.0) and got["track_angle"][5] == (0.0 if k == 0 else -1.0)
    got = run("exact_angle", 0)            # the first pair meets min_angle and does not exit: the second pair's angle is reported
    assert got["track_outlier"].tolist() == [0] and abs(got["track_angle"][0] - np.arctan(0.125)) < 1e-14 and got["track_error"][0] == 0.0
