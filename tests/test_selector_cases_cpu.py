"""The references of tests/test_selectors_gpu.py checked against each other, without a GPU: the plain restatement of
chooseIdx.m, triangulateWithThreshold.m and findGridCorrespondences.m (tests/selector_cases.py) against the C oracle on every
case at every patch size, the distance of every decision from its threshold, and that each case reaches the path it was built
for."""
import numpy as np
import pytest

import selector_cases as SC

NAMES = SC.CASE_NAMES
MARGIN = 1e-9


def test_the_cases_are_the_listed_ones():
    assert tuple(c.name for c in SC.cases()) == NAMES


def _same_as_oracle(c, keys, rows1, rows2, fallback, ref, tag):
    r1, r2, idx, fb = ref
    assert len(r1) == len(keys), (tag, len(r1), len(keys))
    assert fb == fallback, tag
    assert np.array_equal(idx, np.asarray(keys, np.int32).reshape(-1, 2)), tag
    assert np.array_equal(r1, c.t1[rows1, :2]) and np.array_equal(r2, c.t2[rows2, :2]), tag


@pytest.mark.parametrize('name', NAMES)
def test_restatement_equals_the_oracle(orc, name):
    c = SC.case(name)
    K1, K2, T21 = SC.rig()
    for patch in SC.PATCHES:
        th = SC.threshold(name, patch)
        ch = SC.chosen(name, patch)
        _same_as_oracle(c, ch.keys, ch.rows1, ch.rows2, ch.fallback, orc.choose_idx(c.t1, c.t2, K1, K2, T21, patch, th), (name, patch))
    th = SC.threshold(name)
    keys, rows1, rows2, _, fb = SC.plain_threshold(c.t1, c.t2, SC.rig(), th)
    _same_as_oracle(c, keys, rows1, rows2, fb, orc.triangulate_with_threshold(c.t1, c.t2, K1, K2, T21, th), (name, 'threshold'))
    keys, rows1, rows2 = SC.plain_join(c.t1, c.t2)
    _same_as_oracle(c, keys, rows1, rows2, False, orc.find_correspondences(c.t1, c.t2) + (False,), (name, 'join'))


def _clear_of(values, th, tag, but=None):
    """no value within MARGIN (relative) of th; `but`: the index of the one value that is th itself"""
    for i, v in enumerate(values):
        if i == but:
            assert v == th, tag
        else:
            assert abs(v - th) > MARGIN * th, (tag, i, v, th)


@pytest.mark.parametrize('name', NAMES)
def test_margins(name):
    for patch in SC.PATCHES:
        means = [w.mean for w in SC.windows(name, patch) if w.complete]
        _clear_of(means, SC.threshold(name, patch), (name, patch))
    _clear_of(SC.pair_errors(name)[3], SC.threshold(name), (name, 'threshold'))


def test_margins_of_the_boundary_cases():
    """the boundary thresholds lie on one value by construction, and on no other"""
    for name, patch in SC.BOUNDARY:
        th_equal, th_above, at = SC.boundary(name, patch)
        ws = [w for w in SC.windows(name, patch) if w.complete]
        _clear_of([w.mean for w in ws], th_equal, (name, patch), but=[w.at for w in ws].index(at))
        assert th_above > th_equal and np.nextafter(th_above, 0.0) == th_equal
    th_equal, th_above, key = SC.boundary_pair()
    keys, _, _, err = SC.pair_errors(SC.BOUNDARY_PAIR)
    _clear_of(err, th_equal, 'pair', but=keys.index(key))
    assert th_above > th_equal and np.nextafter(th_above, 0.0) == th_equal


# ------------------------------------------------------------------------------------------- what each case reaches
def _accepted(name, patch, th=None):
    th = SC.threshold(name, patch) if th is None else th
    ws = SC.windows(name, patch)
    return [w for w in ws if w.complete and w.mean < th], [w for w in ws if w.complete and not w.mean < th], [w for w in ws if not w.complete]


# the patch sizes at which a case has complete windows on both sides of its threshold (holes: a window of p x p nodes is complete
# with probability 0.81^(p p) or 0.49^(p p))
MIXED_AT = {'full': range(1, 9), 'holes10': range(1, 5), 'holes30': range(1, 3), 'col_gone': range(1, 9), 'col_only_in_1': range(1, 9),
            'col_only_in_2': range(1, 9), 'tail63': range(1, 9), 'tail64': range(1, 9), 'tail65': range(1, 7), 'digits': range(1, 9),
            'dups': range(1, 4)}


def _reach_mixed(name):
    for patch in MIXED_AT[name]:
        acc, rej, _ = _accepted(name, patch)
        assert acc and rej, (name, patch, len(acc), len(rej))
        assert not SC.chosen(name, patch).fallback


def _reach_shared(name):
    for patch in MIXED_AT[name]:
        if patch >= 2:
            prov = SC.providers(name, patch, SC.threshold(name, patch))
            assert any(len(v) >= 2 for v in prov.values()), (name, patch)


def _reach_incomplete(name):
    both = 0
    for patch in SC.PATCHES:
        acc, rej, inc = _accepted(name, patch)
        assert inc, (name, patch)
        both += bool(acc or rej)
        if not (acc or rej):                  # no complete window at all: the fallback, through windows that all miss a node
            assert SC.chosen(name, patch).fallback
    assert both >= 3


def _cols(w):
    return sorted({c for c, _ in w.cand})


def _reach_gap(name):
    """column 5 is not a value of image 1: 4 and 6 are neighbours in the windows"""
    for patch in range(2, 9):
        acc, _, inc = _accepted(name, patch)
        assert not inc
        over = [w for w in acc if 4 in _cols(w) and 6 in _cols(w)]
        assert over and all(5 not in _cols(w) and len(_cols(w)) == patch for w in over), (name, patch)
        ch = SC.chosen(name, patch)
        assert {4, 6} <= {c for c, _ in ch.keys} and 5 not in {c for c, _ in ch.keys}
        assert all(c >= 0 for c, _ in ch.keys)


def _reach_dead_column(name):
    """column 5 is a value of image 1 that image 2 lacks: it is in the windows and every window that holds it is incomplete"""
    for patch in SC.PATCHES:
        ws = SC.windows(name, patch)
        touching = [w for w in ws if 5 in _cols(w)]
        assert touching and not any(w.complete for w in touching)
        assert all(w.complete for w in ws if 5 not in _cols(w))
        ch = SC.chosen(name, patch)
        assert not ch.fallback and 5 not in {c for c, _ in ch.keys}
        if patch <= 5:
            assert 4 in {c for c, _ in ch.keys}
        else:                                 # columns 0..4 are too few for a window: nothing left of column 5 survives
            assert min(c for c, _ in ch.keys) == 6


def _reach_thin(name):
    for patch in SC.PATCHES:
        ch = SC.chosen(name, patch)
        assert ch.fallback == (patch >= 3), patch
        assert (len(ch.means) == 0) == (patch >= 3)
        assert len(ch.keys) == 24
    c = SC.case(name)
    assert SC.chosen(name, 3).rows1 == list(range(24))                 # the join, in table-1 order
    assert SC.chosen(name, 2).keys == sorted(SC.chosen(name, 2).keys, key=lambda k: f'{k[0]}_{k[1]}') != [(int(a), int(b)) for a, b in c.t1[:, 2:4]]


def _reach_exact(name, p):
    c = SC.case(name)
    assert len(c.t1) == len(c.t2) == p * p
    for patch in SC.PATCHES:
        ws = SC.windows(name, patch)
        assert len(ws) == max(p - patch + 1, 0) ** 2 and all(w.complete for w in ws)
        assert SC.chosen(name, patch).fallback == (patch > p)
        assert len(SC.chosen(name, patch).keys) == p * p
    th_equal, th_above, at = SC.boundary(name, p)
    assert at == (0, 0) and th_equal == SC.windows(name, p)[0].mean < SC.TH_FIXED
    eq, ab = SC.chosen(name, p, th_equal), SC.chosen(name, p, th_above)
    assert eq.fallback and not ab.fallback and len(eq.keys) == len(ab.keys) == p * p
    assert eq.rows1 == list(range(p * p))
    if p >= 2:
        assert ab.rows1 != eq.rows1                                    # key order against table-1 order: the flag is not all


def _reach_windows(name, want):
    ws = SC.windows(name, 3)
    assert len(ws) == want and all(w.complete for w in ws)


def _reach_rescue(name):
    c = SC.case(name)
    every = {(int(a), int(b)) for a, b in c.t1[:, 2:4]}
    assert len(every) == 144
    # patch 1: only that point is dropped
    assert set(SC.chosen(name, 1).keys) == every - {SC.OUTLIER}
    dropped_at = [1]
    for patch in range(2, 9):
        acc, rej, inc = _accepted(name, patch)
        assert not inc
        holding = [w for w in acc + rej if SC.OUTLIER in w.cand]
        assert holding and all(w in holding for w in rej)                             # nothing else is ever rejected
        ch = SC.chosen(name, patch)
        if all(w in rej for w in holding):
            # every window that holds the point is rejected: the point is dropped, and each of the other (2 patch - 1)^2 - 1
            # points of those windows is kept through a window that does not hold it
            assert set(ch.keys) == every - {SC.OUTLIER}, patch
            assert len({k for w in holding for k in w.cand}) == (2 * patch - 1) ** 2
            dropped_at.append(patch)
        else:
            # the point's error (2.48 px: half of the 5 px in each image) is averaged with patch^2 - 1 errors of ~0.03 px, and from
            # patch 3 on that mean gets below 0.3: a window that holds the point is accepted, and the point is kept
            assert set(ch.keys) == every, patch
    # patch 3 has both: three of the nine windows that hold the point are rejected, six accepted, and the point is kept through them
    assert dropped_at == [1, 2]
    assert len(_accepted(name, 3)[1]) == 3
    assert all(not _accepted(name, patch)[1] for patch in range(4, 9))


def _reach_all_bad(name):
    for patch in SC.PATCHES:
        acc, rej, inc = _accepted(name, patch)
        assert not acc and not inc and len(rej) == (12 - patch + 1) ** 2
        ch = SC.chosen(name, patch)
        assert ch.fallback and ch.rows1 == list(range(144))
    assert SC.plain_threshold(*SC.case(name)[1:3], SC.rig(), SC.threshold(name))[4]


def _reach_digits(name):
    for patch in SC.PATCHES:
        keys = SC.chosen(name, patch).keys
        assert not SC.chosen(name, patch).fallback
        assert keys != sorted(keys), patch
        pos = {k: i for i, k in enumerate(keys)}
        # the column's digits end in '_', which sorts after a digit: '-10_r' < '-1_r', '10_r' < '1_r', '100_r' < '10_r'
        longer_first = [(a, b) for a in keys for b in keys if a[1] == b[1] and str(a[0]) != str(b[0]) and str(a[0]).startswith(str(b[0]))]
        assert longer_first and all(pos[a] < pos[b] for a, b in longer_first), patch
        assert any(a[0] < 0 for a, _ in longer_first) and any(a[0] > 0 for a, _ in longer_first), patch
        # the row's digits end the string: 'c_-1' < 'c_-10' < 'c_-100', 'c_1' < 'c_10'
        shorter_first = [(a, b) for a in keys for b in keys if a[0] == b[0] and str(a[1]) != str(b[1]) and str(b[1]).startswith(str(a[1]))]
        assert shorter_first and all(pos[a] < pos[b] for a, b in shorter_first), patch
        assert any(a[1] < 0 for a, _ in shorter_first) and any(a[1] > 0 for a, _ in shorter_first), patch
        # and a digit against a sign: 'c_-9' < 'c_0', '-9_r' < '0_r'
        assert all(pos[a] < pos[b] for a in keys for b in keys if a[1] == b[1] and a[0] < 0 <= b[0])


def _reach_duplicates(name):
    c = SC.case(name)
    for t in (c.t1, c.t2):
        ids = [(int(a), int(b)) for a, b in t[:, 2:4]]
        twice = [k for k in set(ids) if ids.count(k) == 2]
        assert len(twice) >= 30
        first = {k: ids.index(k) for k in twice}
        assert all(not np.array_equal(t[i, :2], t[len(ids) - 1 - ids[::-1].index(k), :2]) for k, i in first.items())
    # the join lists a duplicated row of table 1 twice, chooseIdx once
    assert len(SC.plain_join(c.t1, c.t2)[0]) > len(set(SC.plain_join(c.t1, c.t2)[0]))
    ch = SC.chosen(name, 2)
    assert not ch.fallback and len(ch.keys) == len(set(ch.keys))


@pytest.mark.parametrize('name', NAMES)
def test_cases_reach_their_paths(name):
    c = SC.case(name)
    assert c.reaches
    for what in c.reaches:
        head, _, arg = what.partition(':')
        fn = globals()['_reach_' + head]
        fn(name, int(arg)) if arg else fn(name)


def test_patch_sizes_are_told_apart():
    """holes10 at patch 2 and 5 against patch 3 (the default) with the same th: different selections, so a patch argument that
    does not arrive shows"""
    for p in (2, 5):
        got, default = SC.chosen('holes10', p), SC.chosen('holes10', 3, SC.threshold('holes10', p))
        assert not got.fallback and len(got.keys) != len(default.keys)


@pytest.mark.parametrize('name,patch', SC.BOUNDARY)
def test_boundary_is_strict(orc, name, patch):
    c = SC.case(name)
    K1, K2, T21 = SC.rig()
    th_equal, th_above, at = SC.boundary(name, patch)
    only = SC.boundary_keys(name, patch)
    assert only
    _, _, idx_eq, fb_eq = orc.choose_idx(c.t1, c.t2, K1, K2, T21, patch, th_equal)
    _, _, idx_ab, fb_ab = orc.choose_idx(c.t1, c.t2, K1, K2, T21, patch, th_above)
    keys_eq, keys_ab = [tuple(k) for k in idx_eq.tolist()], [tuple(k) for k in idx_ab.tolist()]
    assert not fb_ab and set(only) <= set(keys_ab)
    if name.startswith('exact_'):
        assert fb_eq and len(keys_eq) == len(keys_ab) == patch * patch
    else:
        assert not fb_eq and not set(only) & set(keys_eq) and set(keys_ab) - set(keys_eq) == set(only)
    for th, keys, fb in ((th_equal, keys_eq, fb_eq), (th_above, keys_ab, fb_ab)):
        ch = SC.chosen(name, patch, th)
        assert ch.keys == keys and ch.fallback == fb


def test_boundary_is_strict_for_the_pair_threshold(orc):
    c = SC.case(SC.BOUNDARY_PAIR)
    K1, K2, T21 = SC.rig()
    th_equal, th_above, key = SC.boundary_pair()
    _, _, idx_eq, fb_eq = orc.triangulate_with_threshold(c.t1, c.t2, K1, K2, T21, th_equal)
    _, _, idx_ab, fb_ab = orc.triangulate_with_threshold(c.t1, c.t2, K1, K2, T21, th_above)
    keys_eq, keys_ab = [tuple(k) for k in idx_eq.tolist()], [tuple(k) for k in idx_ab.tolist()]
    assert not fb_eq and not fb_ab
    assert key not in keys_eq and key in keys_ab and [k for k in keys_ab if k != key] == keys_eq
    assert SC.plain_threshold(c.t1, c.t2, SC.rig(), th_equal)[0] == keys_eq
    assert SC.plain_threshold(c.t1, c.t2, SC.rig(), th_above)[0] == keys_ab
