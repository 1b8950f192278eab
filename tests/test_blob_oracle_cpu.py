"""The oracle's detect_largest_blob is split at the sweep image (largest_blob_from_sweep, the counterpart of
cpe_debug_blob_region): the split must not change it.  detect_largest_blob(g) == largest_blob_from_sweep(clahe(lab_l(g)))
on rendered and on noisy frames, and simple_blob_detector's per-threshold records agree with its counts."""
import numpy as np
import pytest


def _frames():
    from cpe_amd import synth
    b = synth.render_batch(2, 480, 640, seed=11, with_gt=False)
    out = [b['left'][0].numpy(), b['right'][1].numpy()]
    rng = np.random.default_rng(3)
    noisy = out[0].astype(np.int32) + rng.integers(-12, 13, size=out[0].shape)
    out.append(np.clip(noisy, 0, 255).astype(np.uint8))
    out.append(rng.integers(0, 256, size=(203, 200)).astype(np.uint8))
    return out


@pytest.mark.parametrize('i', range(4))
def test_largest_blob_split_at_the_sweep_image(orc, i):
    from oracle import stages as S
    g = _frames()[i]
    st, mask, rect, cl, nk = S.detect_largest_blob(g)
    assert np.array_equal(cl, S.clahe(S.lab_l(g)))
    st2, mask2, rect2, nk2 = S.largest_blob_from_sweep(cl)
    assert (st2, nk2) == (st, nk) and np.array_equal(mask2, mask)
    if st == 0:
        assert rect2 == rect
    kp, stats = S.simple_blob_detector(cl)
    kp3, stats3, blobs = S.simple_blob_detector(cl, blobs=True)
    assert np.array_equal(kp, kp3) and np.array_equal(stats, stats3) and len(kp) == nk
    assert [len(b) for b in blobs] == list(stats)
    for b in blobs:
        assert np.isfinite(b).all() and (b[:, 2] > 0).all()
