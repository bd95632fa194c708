"""tests/resize_ref.py's numpy restatement of Pillow's BILINEAR resize against the installed Pillow and against the recorded
fixture (tests/golden/resize_pil.npz), byte for byte: every pair of sides from {1, 2, 3, 5, 8, 13, 16, 17, 31, 40} in width
against the heights (7 -> 7), (9 -> 4), (4 -> 9), (33 -> 2), and the named geometries up to 1920 x 1080 -> 480 x 270 -- over
uniform random, random 0 / 255, constant 0, constant 255 and a ramp along each axis.  The restatement is what the device
tables (tests/test_resize_host.py) and the kernel (tests/test_gpu_resize.py) are then held against."""
import numpy as np
import pytest

from tests import resize_ref as R


def pillow_resize(src, size):
    from PIL import Image

    return np.asarray(Image.fromarray(src).resize(size, Image.BILINEAR))


def test_case_list_covers_what_it_says():
    cases = R.cases()
    geoms = {g for g, _, _ in cases}
    assert len(R.sweep_geometries()) == 400 and set(R.sweep_geometries()) <= geoms and set(R.NAMED) <= geoms
    for g in R.NAMED[:-1]:
        assert {k for gg, k, _ in cases if gg == g} == set(R.KINDS)
    for hs_h in R.HEIGHTS:  # every kind meets every height pair
        assert {k for g, k, _ in cases if (g[1], g[3]) == hs_h} == set(R.KINDS)
    assert len({R.case_key(*c) for c in cases}) == len(cases)


def test_restatement_equals_the_installed_pillow_on_the_sweep():
    """every sweep geometry with EVERY kind (the fixture records one kind per geometry)"""
    bad = []
    for i, g in enumerate(R.sweep_geometries()):
        for kind in R.KINDS:
            src = R.contents(kind, 77 + i, g[0], g[1])[0]
            if not np.array_equal(R.resize(src, g[2:]), pillow_resize(src, g[2:])):
                bad.append((g, kind))
    assert not bad, bad[:10]


@pytest.mark.parametrize("geom", R.NAMED, ids=lambda g: "%dx%d-%dx%d" % g)
def test_restatement_equals_the_installed_pillow_on_the_named_geometries(geom):
    for k, kind in enumerate(R.RANDOM_KINDS if geom == R.LARGE else R.KINDS):
        src = R.contents(kind, 300 + k, geom[0], geom[1])[0]
        got, want = R.resize(src, geom[2:]), pillow_resize(src, geom[2:])
        assert np.array_equal(got, want), (geom, kind, int((got != want).sum()))


def test_batched_restatement_is_the_frames_one_by_one():
    src = R.contents("uniform", 5, 37, 23, frames=3)
    assert not np.array_equal(src[0], src[1])
    got = R.resize(src, (16, 9))
    for n in range(3):
        assert np.array_equal(got[n], pillow_resize(src[n], (16, 9)))
    assert np.array_equal(R.resize(src, (37, 23)), src)


def test_fixture_is_what_the_installed_pillow_and_the_restatement_give():
    meta, arrays = R.load_fixture()
    assert [(tuple(m["geometry"]), m["kind"], m["seed"]) for m in meta] == R.cases()
    hashed = 0
    for m in meta:
        g = tuple(m["geometry"])
        src = R.contents(m["kind"], m["seed"], g[0], g[1])[0]
        got = R.resize(src, g[2:])
        if "sha256" in m:
            hashed += 1
            assert R.hash_only(g, m["kind"]) and m["key"] not in arrays.files
            assert R.sha256(got) == m["sha256"] == R.sha256(pillow_resize(src, g[2:])), m["key"]
        else:
            assert np.array_equal(got, arrays[m["key"]]), m["key"]
    assert hashed == 4
