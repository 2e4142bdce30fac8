"""The back-substitution yardstick without a GPU (tests/backsub_yardstick.py).

(i) The plain float64 restatement of the oracle's back-substitution (bo._back_substitute and the model / candidate / step-norm
lines of bo.solve, camera step from bo._solve_exact, work items from debug_pack) passes every check of the yardstick on every case
and radius of the catalogue (its point step, a product with np.linalg.inv, against the inverse-form bar): the bars, derived from
operation counts, are wide enough for a correct float64 implementation.
(ii) The catalogue contains every branch the kernels take (test_catalogue_coverage)."""
import numpy as np
import pytest

from tests import backsub_yardstick as Y

# The oracle's own camera step (bo._solve_exact: dense float64 Cholesky of S, np.linalg.inv of the damped point blocks) refuses
# radius 1e16 on two problems: S of `regular` and `ragged` is not positive definite in float64 there, and the rank-2 point blocks of
# the single-observation tracks of `ragged` are singular to float64 from radius 1e10 on.  The restatement runs at the largest radius
# of 1e14, 1e12, 1e10, 1e8 the oracle accepts instead; the GPU tests run the library at 1e16.
CPU_RADIUS = {("regular", 1e16): 1e14, ("ragged", 1e16): 1e8}


@pytest.mark.parametrize("name", list(Y.CASES))
def test_float64_restatement_is_inside_every_bar(lib, name):
    arr = Y.case(name)
    items = Y.items_from_pack(arr)
    for radius in Y.CASES[name][1]:
        radius = CPU_RADIUS.get((name, radius), radius)
        inp = Y.oracle_inputs(arr, radius)
        got = Y.float64_restatement(arr, inp, items)
        w = Y.assert_inside(Y.check_all(arr, inp, got), (name, radius), explicit_inverse=True)
        print(name, radius, {k: f"{v[0]:.3f}" for k, v in w.items()})


def test_catalogue_coverage(lib):
    """Taken together the cases contain: items of 1, 2, 3 and 4 tiles, a track of exactly 64 observations, a track head on lane 63,
    a track of length 1, a tile with dead lanes after its last track, a constant point in a tile with variable points, every
    cam_const value 0..3, a camera without observations, every camera model (the five of the reference and the bal9 model) and at
    least ten clamp-branch observations."""
    cov = [Y.coverage(Y.case(n)) for n in Y.CASES]
    union = lambda k: set().union(*(c[k] for c in cov))
    assert union("n_tiles") >= {1, 2, 3, 4}
    for k in ("track64", "head63", "track1", "dead_lanes", "const_in_mixed_tile", "inactive_cam"):
        assert any(c[k] for c in cov), k
    assert union("cam_const") == {0, 1, 2, 3}
    assert union("models") >= {0, 1, 2, 3, 4, 5}
    assert sum(c["clamped"] for c in cov) >= 10
    # the cases that run under all three variants cover the same by themselves, bal9 model aside
    cov = [Y.coverage(Y.case(n)) for n in Y.CASES if Y.CASES[n][2]]
    assert union("n_tiles") >= {1, 2, 3, 4} and union("models") >= {0, 1, 2, 3, 4} and union("cam_const") == {0, 1, 2, 3}
    for k in ("track64", "head63", "track1", "dead_lanes", "const_in_mixed_tile", "inactive_cam"):
        assert any(c[k] for c in cov), k
    # single-observation tracks (rank-2 point blocks) are in the catalogue, at the radii stated above and in test_gpu_backsub.py
    assert (np.bincount(Y.case("ragged")["obs_pt"]) == 1).sum() > 5 and CPU_RADIUS[("ragged", 1e16)] == 1e8
