"""The host side of the raw-frame entry point (cpe_amd/experiment.py: getUniqueName.m, parseImgInfo.m, imread's element
types) and the declaration of the fused pre-step in the C ABI.  No GPU."""
import ctypes as C
import warnings

import numpy as np
import pytest


def test_parse_img_info():
    from cpe_amd import experiment
    with warnings.catch_warnings():
        warnings.simplefilter('error')                  # well-formed names give no warning
        a = experiment.parse_img_info(['00', '1-8', '-1-4', '123'])
    assert a.dtype == np.float64 and a.tolist() == [[0, 0], [1, -8], [-1, -4], [12, 3]]     # greedy first group, as MATLAB's regexp
    with pytest.warns(UserWarning, match='ab'):
        b = experiment.parse_img_info(['ab', '-10'])
    assert b.tolist() == [[0, 0], [-1, 0]]
    assert experiment.parse_img_info([]).shape == (0, 2)


def test_unique_names(tmp_path):
    from cpe_amd import experiment
    for f in ('1-2L.png', '1-2R.png', '00L.png', '00R.png', '-10L.png', 'L.png', 'abL.PNG', '07L.jpg', '3L.png.txt', 'R.png', '12l.png',
              '5LL.png'):
        (tmp_path / f).write_bytes(b'')
    # 'L.png' has 5 characters: an empty stem, as in getUniqueName.m:11-14; a 4-character name cannot end in 'L.png'
    (tmp_path / '.png').write_bytes(b'')
    assert experiment.unique_names(str(tmp_path)) == sorted(['', '-10', '00', '1-2', '5L'])
    assert experiment.unique_names(str(tmp_path))[0] == ''


def test_read_raw_image_dtypes(tmp_path):
    from PIL import Image
    from cpe_amd import experiment
    rng = np.random.default_rng(0)
    g8 = rng.integers(0, 256, (5, 7), dtype=np.uint8)
    g16 = rng.integers(0, 65536, (5, 7)).astype(np.uint16); g16[0, :2] = (0, 65535)
    rgb = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    Image.fromarray(g8).save(tmp_path / 'g8.png')
    Image.fromarray(g16).save(tmp_path / 'g16.png')
    Image.fromarray(rgb).save(tmp_path / 'rgb.png')
    for name, want in (('g8', g8), ('g16', g16), ('rgb', rgb)):
        got = experiment.read_raw_image(str(tmp_path / f'{name}.png'))
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), name
    with pytest.raises(FileNotFoundError, match='nope.png'):
        experiment.read_raw_image(str(tmp_path / 'nope.png'))


def test_read_raw_image_alpha_and_wide_grey(tmp_path):
    """grey with alpha reads as grey (imread returns alpha apart); a 32-bit grey image is narrowed to uint16 only when every
    value fits, never wrapped"""
    from PIL import Image
    import cpe_amd
    from cpe_amd import experiment
    g8 = np.arange(35, dtype=np.uint8).reshape(5, 7)
    Image.merge('LA', (Image.fromarray(g8), Image.fromarray(np.full((5, 7), 9, np.uint8)))).save(tmp_path / 'la.png')
    got = experiment.read_raw_image(str(tmp_path / 'la.png'))
    assert got.dtype == np.uint8 and np.array_equal(got, g8)
    wide = np.array([[0, 65535, 300], [1, 2, 3]], dtype=np.int32)
    Image.fromarray(wide, mode='I').save(tmp_path / 'ok.tif')
    got = experiment.read_raw_image(str(tmp_path / 'ok.tif'))
    assert got.dtype == np.uint16 and np.array_equal(got, wide)
    wide[1, 1] = 65536
    Image.fromarray(wide, mode='I').save(tmp_path / 'big.tif')
    with pytest.raises(cpe_amd.lib.CpeError, match='65536'):
        experiment.read_raw_image(str(tmp_path / 'big.tif'))


def test_prestep_symbol_declared():
    import cpe_amd
    assert 'cpe_matlab_prestep_batch' in cpe_amd.lib.declared_symbols()
    res, args = cpe_amd.lib._SIGS['cpe_matlab_prestep_batch']
    assert res is C.c_int32 and len(args) == 11 and args[9] is C.c_int64
    hdr = open(cpe_amd.lib._HERE + '/../include/cpe.h').read()
    for k, v in (('U8', 0), ('U16', 1), ('F32', 2), ('F64', 3)):
        assert f'#define CPE_PIX_{k} {v}\n' in hdr
    from cpe_amd import iotool
    import torch
    assert iotool._PIX[torch.uint8] == 0 and iotool._PIX[torch.int16] == 1 and iotool._PIX[torch.float32] == 2 and iotool._PIX[torch.float64] == 3


def test_im2uint8_u16_integer_forms():
    """the kernel's (x + 128) / 257 is round(x / 257) for all 65536 values (257 is odd: no ties), and so is the multiply-shift form"""
    x = np.arange(65536, dtype=np.int64)
    a = (x + 128) // 257
    assert np.array_equal(a, np.floor(x / 257.0 + 0.5).astype(np.int64)) and not np.any((2 * x) % 514 == 257)
    assert np.array_equal(a, ((x + 128) * 65281) >> 24) and a.max() == 255 and a.min() == 0
