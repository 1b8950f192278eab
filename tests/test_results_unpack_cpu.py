"""api.unpack_results on hand-built records: the decoder of the packed results (include/cpe.h, "Packed results") needs neither
a GPU nor the library, returns exactly the objects the per-frame interface returns, and refuses what does not follow the
layout.  The records are assembled here field by field from the header's text, not with the package's helpers."""
import struct

import numpy as np
import pytest


def _record(status, center, xy, ids, rows, cols):
    """rows / cols: lists of (equation of 6 floats, [(x, y), ...]) -> bytes of one record"""
    lines = list(rows) + list(cols)
    n_row_pts = sum(len(p) for _, p in rows)
    n_col_pts = sum(len(p) for _, p in cols)
    b = struct.pack('<8i', status, len(xy), len(rows), len(cols), n_row_pts, n_col_pts, 0, 0)
    b += struct.pack('<2d', *center)
    for x, y in xy:
        b += struct.pack('<2d', x, y)
    for a, c in ids:
        b += struct.pack('<2i', a, c)
    for eq, _ in lines:
        b += struct.pack('<6d', *eq)
    start = [0]
    for _, p in lines:
        start.append(start[-1] + len(p))
    b += struct.pack(f'<{len(start)}i', *start)
    if len(start) % 2:
        b += struct.pack('<i', 0)
    for _, p in lines:
        for x, y in p:
            b += struct.pack('<2d', x, y)
    assert len(b) % 8 == 0
    return b


def _pack(records):
    off = np.zeros(len(records) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in records])
    return off, np.frombuffer(b''.join(records), np.uint8).copy()


def _eq(k):
    return [0.001 * k, -0.5 + k, 100.25 * k, -50.0, 690.5, 740.5]


GOOD = dict(status=0, center=(320.5, 240.25), xy=[(10.5, 20.25), (30.0, 40.125), (1e-3, 479.999)], ids=[(0, -1), (0, 0), (1, 2)],
            rows=[(_eq(1), [(1.0, 2.0), (3.0, 4.5)]), (_eq(2), [(5.0, 6.0)]), (_eq(3), [(7.0, 8.0), (9.0, 10.0), (11.0, 12.5), (13.0, 14.0)])],
            cols=[(_eq(4), [(1.5, 2.5), (3.5, 4.5), (5.5, 6.5)]), (_eq(5), [(0.1, 0.2)])])
EMPTY = dict(status=1, center=(0.0, 0.0), xy=[], ids=[], rows=[], cols=[])
FAILED = dict(status=4, center=(0.0, 0.0), xy=[], ids=[], rows=[(_eq(6), [(2.0, 3.0)]), (_eq(7), [(4.0, 5.0), (6.0, 7.0)])],
              cols=[(_eq(8), [(8.0, 9.0)])])
ZERO_LINE = dict(status=0, center=(5.0, 6.0), xy=[(5.0, 6.0)], ids=[(0, 0)], rows=[(_eq(1), [(5.0, 6.0)]), (_eq(2), [])],
                 cols=[(_eq(3), []), (_eq(4), [(5.0, 6.0)])])


def _want_tables(lines, prefix):
    return {'points': {f'{prefix}{i + 1}': [tuple(p) for p in pts] for i, (_, pts) in enumerate(lines)},
            'equations': {f'{prefix}{i + 1}': list(eq) for i, (eq, _) in enumerate(lines)}}


def _check(rec, spec):
    assert rec.status == spec['status'] and isinstance(rec.status, int)
    assert rec.n == len(spec['xy'])
    assert rec.center.dtype == np.float64 and rec.center.tolist() == list(spec['center'])
    assert rec.xy.dtype == np.float64 and rec.xy.shape == (len(spec['xy']), 2) and rec.xy.tolist() == [list(p) for p in spec['xy']]
    assert rec.id.dtype == np.int32 and rec.id.shape == (len(spec['ids']), 2) and rec.id.tolist() == [list(p) for p in spec['ids']]
    for got, want in ((rec.rows, _want_tables(spec['rows'], 'row')), (rec.cols, _want_tables(spec['cols'], 'col'))):
        assert got == want
        assert list(got) == ['points', 'equations']
        assert list(got['points']) == list(want['points']) and list(got['equations']) == list(want['equations'])   # key order
        for pts in got['points'].values():
            assert type(pts) is list and all(type(p) is tuple and type(p[0]) is float and type(p[1]) is float for p in pts)
        for eq in got['equations'].values():
            assert type(eq) is list and len(eq) == 6 and all(type(v) is float for v in eq)


def test_hand_built_records_decode_to_the_per_frame_objects(cpe):
    specs = [GOOD, EMPTY, FAILED, ZERO_LINE, GOOD]
    off, payload = _pack([_record(**s) for s in specs])
    assert int(off[1]) == 48 + 24 * 3 + 48 * 5 + 8 * 3 + 16 * 11        # the size formula of the header, by hand
    assert int(off[2] - off[1]) == 48 + 8                                # empty frame: header, centre, start[0] and its padding
    got = cpe.api.unpack_results(off, payload)
    assert len(got) == len(specs)
    for rec, spec in zip(got, specs):
        _check(rec, spec)
    # a longer payload than offsets[n] is fine (a reused staging buffer); the result owns its data
    longer = np.concatenate([payload, np.full(64, 0xA5, np.uint8)])
    again = cpe.api.unpack_results(off, longer)
    longer[:] = 0
    payload[:] = 0
    for rec, spec in zip(again, specs):
        _check(rec, spec)
    for rec, spec in zip(got, specs):
        _check(rec, spec)


def test_planar_ids_are_kept_in_their_stored_order(cpe):
    """the planar script's ids are (row, col): the decoder hands the pairs on as stored, and make_json prints them so"""
    spec = dict(GOOD, ids=[(-1, 0), (0, 0), (2, 1)])
    off, payload = _pack([_record(**spec)])
    rec = cpe.api.unpack_results(off, payload, target='plane')[0]
    _check(rec, spec)
    import json
    d = json.loads(cpe.api.make_json(rec.center, rec.xy, rec.id))
    assert [p['id'] for p in d['points']] == [[-1, 0], [0, 0], [2, 1]]
    with pytest.raises(ValueError):
        cpe.api.unpack_results(off, payload, target='sphere')


def test_decoder_refuses_what_does_not_follow_the_layout(cpe):
    recs = [_record(**GOOD), _record(**FAILED)]
    off, payload = _pack(recs)
    U = cpe.api.unpack_results
    assert len(U(off, payload)) == 2
    with pytest.raises(ValueError):                      # short payload: by one byte, by half, empty
        U(off, payload[:-1])
    with pytest.raises(ValueError):
        U(off, payload[:len(payload) // 2])
    with pytest.raises(ValueError):
        U(off, payload[:0])
    with pytest.raises(ValueError):                      # non-monotone offsets
        U(np.array([0, off[2], off[1]], np.int64), payload)
    with pytest.raises(ValueError):                      # a repeated offset (a record of no bytes)
        U(np.array([0, off[1], off[1], off[2]], np.int64), payload)
    with pytest.raises(ValueError):                      # unaligned offsets
        U(np.array([0, off[1] + 4, off[2]], np.int64), payload)
    with pytest.raises(ValueError):                      # not starting at 0
        U(np.array([8, off[1], off[2]], np.int64), payload)
    with pytest.raises(ValueError):                      # wrong types
        U(off.astype(np.int32), payload)
    with pytest.raises(ValueError):
        U(off, payload.astype(np.int8))
    with pytest.raises(ValueError):
        U(np.zeros(0, np.int64), payload)
    # a count that overruns its record: each of the five counts in turn, and a negative one
    for field in range(1, 6):
        for delta in (1, 1000, -100000):
            bad = payload.copy()
            v = bad[4 * field:4 * field + 4].view('<i4')
            v[0] += delta
            with pytest.raises(ValueError):
                U(off, bad)
    # counts that fill the record but disagree with the start table (one row point moved to the columns)
    bad = payload.copy()
    hdr = bad[:32].view('<i4')
    hdr[4] -= 1; hdr[5] += 1
    with pytest.raises(ValueError):
        U(off, bad)
    bad = payload.copy()                                 # a start table that runs backwards
    p = 48 + 24 * 3 + 48 * 5
    st = bad[p:p + 24].view('<i4')
    st[1], st[2] = st[2], st[1] - 5
    with pytest.raises(ValueError):
        U(off, bad)
    bad = payload.copy()                                 # reserved header words are zero
    bad[24] = 1
    with pytest.raises(ValueError):
        U(off, bad)
    assert len(U(np.array([0], np.int64), payload[:0])) == 0     # no frames: nothing to decode
