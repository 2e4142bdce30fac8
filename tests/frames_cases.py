"""Inputs shared by tests/test_frames_cpu.py and tests/test_gpu_frames.py: the two-view scenes of the verification tests (the
construction of test_match_verify_and_two_view_init_recover_the_generating_pose of tests/test_gpu_match.py, key points rounded to
float32), and the frame set that holds all of them with the pair list of the one call."""
import functools

import numpy as np

from tests import fund_yardstick as YF
from tests import match_yardstick as Y

# (related, unrelated) key points of either frame; 12/5 gives 12 matches, below min_matches: status 2
SIZES = ((24, 9), (40, 17), (12, 5), (600, 257))


@functools.lru_cache(None)
def scene(n_rel, n_other):
    """dict(desc_a, desc_b [n][128] uint8, kp_a, kp_b [n][2] float32, perm): frame b in another order"""
    rng = np.random.default_rng(77 + n_rel)
    xa, xb, _, _ = YF.make_pair(n_rel, 0.0, 0.0, seed=4242, baseline=2.2)
    da = Y.sift_like(rng, n_rel)
    desc_a = np.concatenate([da, Y.sift_like(rng, n_other)])
    desc_b = np.concatenate([Y.perturb(rng, da), Y.sift_like(rng, n_other)])
    kp_a = np.concatenate([xa, rng.uniform(0, 2 * YF.K[0, 2], (n_other, 2))])
    kp_b = np.concatenate([xb, rng.uniform(0, 2 * YF.K[0, 2], (n_other, 2))])
    perm = rng.permutation(len(desc_b))
    return dict(desc_a=desc_a, desc_b=desc_b[perm], kp_a=kp_a.astype(np.float32), kp_b=kp_b[perm].astype(np.float32), perm=perm)


@functools.lru_cache(None)
def scene_set():
    """(key_ptr, keys [N][4] float32, desc [N][128]) of the frames a0 b0 a1 b1 a2 b2 a3 b3 and one empty frame (index 8)"""
    ks, ds, ptr = [], [], [0]
    for n_rel, n_other in SIZES:
        s = scene(n_rel, n_other)
        for kp, d in ((s["kp_a"], s["desc_a"]), (s["kp_b"], s["desc_b"])):
            ks.append(np.concatenate([kp, np.ones((len(kp), 2), np.float32)], 1)); ds.append(d); ptr.append(ptr[-1] + len(d))
    ptr.append(ptr[-1])
    return np.array(ptr, np.int64), np.ascontiguousarray(np.concatenate(ks), np.float32), np.ascontiguousarray(np.concatenate(ds))


# the one call: the four scenes, a pair a == b, a pair with the empty frame on either side, scene 1 again under another seed, and
# scene 0 with a max_error of its own
PAIR_A = np.array([0, 2, 4, 6, 2, 8, 1, 2, 0], np.int32)
PAIR_B = np.array([1, 3, 5, 7, 2, 1, 8, 3, 1], np.int32)
PAIR_SEED = np.array([0, 0, 0, 0, 0, 0, 0, 12345, 0], np.uint32)
PAIR_MAX_ERROR = np.array([4.0, 4.0, 4.0, 4.0, 4.0, 4.0, 4.0, 4.0, 0.5])
