"""The inputs of the end-to-end and the rotation test of tests/test_gpu_desc.py, and what can be said about them without a GPU
(tests/test_desc_cpu.py checks these on the CPU): the pair of translated images, which keypoints are eligible, the comparator (the
host programs' descriptors through tests/match_yardstick.py), the rotated pair and the deviation that its two gradient planes cause
in the float32 restatement."""
import functools

import numpy as np

from tests import desc_host_driver as DH
from tests import desc_yardstick as D
from tests import match_yardstick as M
from tests import sift_host_driver as H
from tests import sift_yardstick as Y

# The 96 x 80 canvas of the translation test of test_gpu_sift.py leaves no room once the descriptor's footprint (up to 10.6 sigma)
# is added to the filter reach: checked on the CPU, fewer than 20.  The richer canvas: the 300 x 260 catalogue image on 400 x 360.
E2E_NAME, E2E_CANVAS, E2E_SHIFTS = "e300x260", (400, 360), ((8, 8), (12, 12))
FOOT = 2.5 * np.sqrt(2.0) * 3.0          # of a descriptor, in sigma: the farthest cell centre (1.5 sqrt(2) spt) plus the box (sqrt(2) spt), spt = 3 sigma


def e2e_images():
    return [Y.translated(dx, dy, E2E_NAME, E2E_CANVAS) for dx, dy in E2E_SHIFTS]


def eligible(loc, keys, first_octave=-1):
    """[n] bool: the keypoint's descriptor and orientation windows, the gradient's neighbours and, below them, every filter on the
    way stay clear of every border, in this image and at the shifted place in the other (shift 8 >> octave pixels either way)"""
    geo, reach = Y.geometry(E2E_CANVAS[0], E2E_CANVAS[1], first_octave, 4), Y.filter_reach(first_octave, 4)
    out = np.zeros(len(loc), bool)
    for k, (o, j, r, c) in enumerate(np.asarray(loc).tolist()):
        w, h = geo[o]
        sigma = float(keys[k][2]) / 2.0 ** (first_octave + o)
        m = reach[o] + 2 + int(np.ceil(FOOT * sigma)) + (8 >> o)
        out[k] = m <= r < h - m and m <= c < w - m
    return out


def counterpart(la, lb):
    s = 8 >> int(la[0])
    return tuple(la[:2]) == tuple(lb[:2]) and int(lb[2]) == int(la[2]) + s and int(lb[3]) == int(la[3]) + s


def count_matches(loc_a, loc_b, keys_a, keys_b, matches):
    ea, eb = eligible(loc_a, keys_a), eligible(loc_b, keys_b)
    correct = wrong = 0
    for a, b in np.asarray(matches).reshape(-1, 2).tolist():
        if ea[a] or eb[b]:
            if counterpart(loc_a[a], loc_b[b]):
                correct += 1
            else:
                wrong += 1
    return correct, wrong


def e2e_comparator(directory, flags=("-O2",)):
    """(correct, wrong) matches among the eligible keypoints with the host programs' descriptors, through match_yardstick on the CPU"""
    sift_exe, desc_exe = H.build(directory, flags=list(flags)), DH.build(directory, flags=list(flags))
    out = []
    for img in e2e_images():
        d, s = DH.run_image(sift_exe, desc_exe, directory, img, Y.options())
        out.append((s["loc"], s["keys"], d["desc"]))
    m = M.run_pair(out[0][2], out[1][2])["matches"]
    return count_matches(out[0][0], out[1][0], out[0][1], out[1][1], m)


# ------------------------------------------------------------------------------------------------- rotation
@functools.lru_cache(None)
def rotation_images():
    a = Y.blobs(64, 64, 21, Y._bands(64, 64, [(1, [5, 7]), (1, [6, 9])]))
    return a, np.ascontiguousarray(np.rot90(a))


def rotation_pairs(loc_a, loc_b, octave=0, size=64, margin=2):
    """(index in a, index in b) of octave-0 keypoints found in both: np.rot90 sends pixel (r, c) to (size - 1 - c, r)"""
    at = {tuple(l): k for k, l in enumerate(np.asarray(loc_b).tolist())}
    out = []
    for k, (o, j, r, c) in enumerate(np.asarray(loc_a).tolist()):
        if o != octave or min(r, c) < margin or max(r, c) > size - 1 - margin:
            continue
        q = at.get((o, j, size - 1 - c, r))
        if q is not None:
            out.append((k, q))
    return out


def quarter_turn_error(wa, wb):
    d = float(wa) - float(wb)
    return min(abs((d - s * np.pi / 2 + np.pi) % (2 * np.pi) - np.pi) for s in (1, -1))


@functools.lru_cache(None)
def rotation_plane_deviation():
    """16 times the largest deviation from a quarter turn between the float32 restatement's orientations of the two images: what the
    different order of the two filter passes leaves in the two gradient planes, and through them in w"""
    a, b = rotation_images()
    ra, rb = (Y.reference(x, False, first_octave=0) for x in (a, b))
    worst = 0.0
    pl = [D.planes_of(r["pyramid"][0][0]) for r in (ra, rb)]
    wa, wb = ([float(D.orientation(p[j], key, D.F)["w"]) if o == 0 else 0.0
               for (o, j, _, _), key in zip(r["loc"].tolist(), D.octave_keys(r["loc"], r["off"].astype(D.F), 0))] for r, p in zip((ra, rb), pl))
    pairs = rotation_pairs(ra["loc"], rb["loc"])
    for i, j in pairs:
        worst = max(worst, quarter_turn_error(wa[i], wb[j]))
    return 16 * worst
