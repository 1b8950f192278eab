"""The reference and the cases of tests/index_shift_cases.py, checked without a GPU: the numbers its docstring states, the
margins that let the GPU test compare integers exactly, and the chain fit -> re-number -> refit stated with
ref_projector_model."""
import numpy as np
import pytest

import index_shift_cases as SC
import plane_fit_cases as PC
import proj_model_cases as M


def test_symbol_is_declared(cpe):
    assert 'cpe_index_shift_batch' in cpe.lib.declared_symbols()
    assert 'cpe_index_shift_batch' in cpe.lib._SIGS
    assert [n for n, _ in cpe.lib.CpeIndexShiftParams._fields_] == ['win', 'tau', 'min_score', 'swap']
    assert cpe.fit.SHIFT_MAX_WIN == SC.MAX_WIN and (cpe.fit.SHIFT_SHIFTED, cpe.fit.SHIFT_WEAK, cpe.fit.SHIFT_EDGE) == (1, 2, 4)


@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('table', ['model', 'rig', 'noisy'])
def test_shifted_frames_are_found(seed, table):
    """(-1, 0) on the frames 3 and 7, (0, 0) elsewhere, 225 at the right shift and 0 at every other candidate, for tau 0.5, 1, 2"""
    import table_tri_cases as TC
    X, I, cnt = PC.pack(M.shifted_frames(seed))
    t = dict(model=SC.model_table, rig=lambda s: TC.rig_table(-16, 16), noisy=lambda s: TC.noisy_table(0))[table](seed)
    for tau in (0.5, 1.0, 2.0):
        r = SC.ref_index_shift(X, I, cnt, t['P'], t['status'], t['lo'], t['hi'], tau=tau)
        want = np.zeros((12, 2), np.int32)
        want[list(M.SHIFTED), 0] = -1
        assert np.array_equal(r['shift'], want)
        assert (r['score'][..., 0] == 225).all() and not r['score'][..., 1].any() and (r['score'][..., 3] == 225).all()
        assert (r['scores'].sum(1) == 450).all()                  # nothing but the two winners
        assert np.array_equal(r['flags'][:, 0] == SC.SHIFTED, want[:, 0] != 0) and not r['flags'][:, 1].any()
        assert np.array_equal(r['idx'][:, :225], I[:, :225] + want[:, None, :]) and not r['idx'][:, 225:].any()
        assert r['margin'] > 1e-6


@pytest.mark.parametrize('name', list(SC.cases()))
def test_margin(name):
    r = SC.reference(name)
    assert r['margin'] > 1e-6, f'{name}: a residual lies within {r["margin"]:.2e} tau of the band'
    assert r['rms_tol'] < 1e-10


def test_cases_cover_what_they_name():
    R = SC.reference
    assert R('window 1 1')['flags'][0, 0] == SC.EDGE | SC.SHIFTED and R('window 1 1')['flags'][1].tolist() == [SC.WEAK, SC.WEAK]
    assert R('window 2 5')['shift'][1].tolist() == [0, 3]
    assert R('counts')['score'][:, 0, 3].tolist() == [0, 0, 1, 63, 64, 65] and R('counts')['shift'][:, 0].tolist() == [0, 0, 0, -1, -1, -1]
    assert R('counts 2048 3000')['score'][:, :, 0].tolist() == [[2048, 2048], [2048, 2048]]
    assert R('counts 2048 3000')['shift'].tolist() == [[0, 1], [0, 2]]
    assert R('L 1')['score'][:, 0, 0].tolist() == [25, 25] and R('L 1')['shift'][:, 0].tolist() == [0, 2]
    assert R('garbage indices')['score'][0, :, 0].tolist() == [219, 219]
    assert R('winner refused')['score'][0, 0].tolist() == [0, 0, 0, 50] and R('winner refused')['flags'][0, 0] == SC.WEAK
    assert np.array_equal(R('transposed swap 1')['scores'], R('three frames')['scores'])
    assert not np.array_equal(R('swap 1')['scores'], R('three frames')['scores'])
    assert (R('min_score 226')['flags'] == SC.WEAK).all() and (R('min_score 226')['score'][..., 0] == 225).all()
    assert not R('min_score 0 empty')['flags'].any()
    assert (R('wide band 6.0')['flags'] == SC.WEAK).all() and (R('wide band 6.0')['score'][..., 1] == 225).all()
    t = R('ties and leads')
    assert t['score'][:, 0, :2].tolist() == [[100, 100], [100, 100], [120, 80], [120, 60], [100, 100]]
    assert t['shift'][:, 0].tolist() == [0, 0, 0, -1, 0] and t['flags'][:, 0].tolist() == [SC.WEAK, SC.WEAK, SC.WEAK, SC.SHIFTED, SC.WEAK]
    # the winners behind the forced zeros: 0 where it is part of the tie, else the smaller |d|, else the smaller d
    sc = t['scores'][:, :9]
    assert sc[0, 3] == sc[0, 4] == 100 and sc[1, 3] == sc[1, 5] == 100 and sc[4, 2] == sc[4, 6] == 100


def test_chain_fit_renumber_refit():
    """ref_projector_model(tau = 1), its table, ref_index_shift, ref_projector_model on the re-numbered indices from the first
    model: no residual is trimmed and the model is the clean fit's, at the reference's tolerance"""
    X, I, cnt = PC.pack(M.shifted_frames(0))
    first = M.ref_projector_model(X, I, cnt, -12, 12, tau=M.TAU)
    assert first['frame_counts'][list(M.SHIFTED), 1].tolist() == [225, 225]
    t = SC.model_table(0)
    sh = SC.ref_index_shift(X, I, cnt, t['P'], t['status'], t['lo'], t['hi'], tau=M.TAU)
    refit = M.ref_projector_model(X, sh['idx'], cnt, -16, 16, tau=M.TAU, x0=first['x'])
    clean = M.reference('cylinder 12')
    assert refit['status'] == 0 and refit['rounds'] == 0 and refit['kept'].tolist() == [2700, 2700]
    assert not refit['frame_counts'][:, [1, 3]].any()
    d = np.abs(refit['x'] - clean['x']).max()
    print(f'refit against the clean fit: {d:.2e} (tol {clean["tol"]:.2e})')
    assert d <= clean['tol']
