"""Row f-3: the undistortion pre-step of the reference's CLI entry point, mirror of utils/iotool.py.

    load_camera_data(json_path)                 iotool.py:8-20   (camera JSON written by createCameraDataJSON.m:7-12)
    undistort_image(image, camera_params)       iotool.py:22-39  (cv2.undistort, bilinear)
    Undistorter(camera_params, h, w, device)    the batched form: the fixed-point map is built once per camera
                                                (cv2.undistort rebuilds it for every image), frames are one gather pass

    Undistorter(..., interp='cubic') /         the MATLAB entry point's pre-step instead: undistortImage(I, cameraParams,
    undistort_image(..., interp='cubic')        'cubic') of utils/preProcessing.m:3-4 (distortPoints map, cubic convolution)

    StereoPrestep(cam_l, cam_r, h, w, device)   utils/preProcessing.m:3-9 for chunks of raw stereo frames in one kernel per
    preprocessing(img_l, img_r, cam_l, cam_r)   camera: im2uint8 (uint8 / uint16 / single / double) + cubic undistortion +
                                                rgb2gray, written as the frame-major pairs FramePipeline reads in place

The planar entry module (python_grid_detection_plane.py) and the cylinder one call the bilinear form for every image of a
folder.  No CPU fallback: the HIP library does the work."""
import ctypes as C
import json

import numpy as np
import torch

from . import lib as _lib


def load_camera_data(json_path):
    """-> (LeftCamera, RightCamera) dicts with IntrinsicMatrix, RadialDistortion, TangentialDistortion"""
    with open(json_path, 'r') as f:
        camera_data = json.load(f)
    return camera_data['LeftCamera'], camera_data['RightCamera']


def camera_arrays(camera_params):
    """K (3x3 f64) and the coefficient vector exactly as iotool.py:33-36 hands them to OpenCV:
    hstack((RadialDistortion, TangentialDistortion)) -- read by OpenCV as (k1, k2, p1, p2[, k3]) whatever it holds"""
    K = np.array(camera_params['IntrinsicMatrix'], dtype=np.float64).reshape(3, 3)
    dist = np.hstack((np.asarray(camera_params['RadialDistortion'], dtype=np.float64).ravel(),
                      np.asarray(camera_params['TangentialDistortion'], dtype=np.float64).ravel()))
    return K, dist


class Undistorter:
    """undistortion map of one camera, resident on the GPU.  interp='linear': cv2.undistort (fixed-point map in the
    CV_16SC2 + CV_16UC1 layout, bilinear); interp='cubic': MATLAB's undistortImage(I, cameraParams, 'cubic') -- the camera
    JSON's matrix read with MATLAB's 1-based principal point, RadialDistortion (2 or 3 terms) and TangentialDistortion kept
    apart, float32 source coordinates, cubic convolution, fill value 0."""

    def __init__(self, camera_params, h, w, device='cuda:0', interp='linear'):
        if interp not in ('linear', 'cubic'):
            raise _lib.CpeError(f"Undistorter: interp must be 'linear' or 'cubic' (got {interp!r})")
        self.h, self.w, self.device, self.interp = int(h), int(w), torch.device(device), interp
        K, dist = camera_arrays(camera_params)
        self.K = np.ascontiguousarray(K)
        L = _lib.load()
        if interp == 'cubic':
            radial = np.ascontiguousarray(np.asarray(camera_params['RadialDistortion'], dtype=np.float64).ravel())
            tang = np.ascontiguousarray(np.asarray(camera_params['TangentialDistortion'], dtype=np.float64).ravel())
            if radial.size not in (2, 3) or tang.size != 2:
                raise _lib.CpeError('MATLAB camera parameters hold 2 or 3 radial and 2 tangential coefficients')
            self.map = torch.empty((self.h, self.w, 2), dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(L.cpe_undistort_map_matlab(self.K.ctypes.data_as(C.c_void_p), radial.ctypes.data_as(C.c_void_p),
                                                      int(radial.size), tang.ctypes.data_as(C.c_void_p), self.h, self.w,
                                                      self.map.data_ptr(), torch.cuda.current_stream().cuda_stream),
                           'cpe_undistort_map_matlab')
            return
        if dist.size not in (0, 4, 5, 8, 12):
            raise _lib.CpeError(f'{dist.size} distortion coefficients: OpenCV takes 4, 5, 8 or 12')
        self.dist = np.ascontiguousarray(dist)
        self.map_xy = torch.empty((self.h, self.w, 2), dtype=torch.int16, device=self.device)
        self.map_f = torch.empty((self.h, self.w), dtype=torch.int16, device=self.device)   # bit pattern of u16
        with torch.cuda.device(self.device):
            _lib.check(L.cpe_undistort_map(self.K.ctypes.data_as(C.c_void_p), self.dist.ctypes.data_as(C.c_void_p),
                                           int(self.dist.size), self.h, self.w, self.map_xy.data_ptr(), self.map_f.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), 'cpe_undistort_map')

    def __call__(self, frames, out=None):
        """frames u8 [n,h,w] (or [h,w]) on the device -> undistorted frames, same shape"""
        single = frames.dim() == 2
        f = frames.unsqueeze(0) if single else frames
        if f.dtype != torch.uint8 or f.shape[1:] != (self.h, self.w) or f.device != self.device or not f.is_contiguous():
            raise _lib.CpeError('Undistorter: frames must be contiguous u8 [n,h,w] on the map\'s device')
        dst = torch.empty_like(f) if out is None else out
        L = _lib.load()
        with torch.cuda.device(self.device):
            s = torch.cuda.current_stream().cuda_stream
            if self.interp == 'cubic':
                _lib.check(L.cpe_remap_cubic_batch(f.data_ptr(), f.shape[0], self.h, self.w, self.map.data_ptr(), 0,
                                                   dst.data_ptr(), s), 'cpe_remap_cubic_batch')
            else:
                _lib.check(L.cpe_remap_bilinear_batch(f.data_ptr(), f.shape[0], self.h, self.w, self.map_xy.data_ptr(),
                                                      self.map_f.data_ptr(), dst.data_ptr(), s), 'cpe_remap_bilinear_batch')
        return dst[0] if single else dst


def undistort_image(image, camera_params, device='cuda:0', interp='linear'):
    """reference signature (iotool.py:22): numpy u8 image [h,w] or [h,w,c] -> undistorted numpy image.
    (Channels are independent in cv2.undistort / undistortImage; they are processed as a batch of planes.)
    interp='cubic' = the MATLAB entry point's undistortImage(I, cameraParams, 'cubic') (preProcessing.m:3-4)."""
    img = np.array(image, copy=True, order='C')     # (PIL / MATLAB hand over read-only buffers)
    if img.dtype != np.uint8 or img.ndim not in (2, 3):
        raise _lib.CpeError('undistort_image: u8 image [h,w] or [h,w,c] expected')
    planes = img[None] if img.ndim == 2 else np.ascontiguousarray(np.moveaxis(img, 2, 0))
    und = Undistorter(camera_params, img.shape[0], img.shape[1], device, interp)
    out = und(torch.from_numpy(planes).to(und.device)).cpu().numpy()
    return out[0] if img.ndim == 2 else np.ascontiguousarray(np.moveaxis(out, 0, 2))


_PIX = {torch.uint8: _lib.const.PIX_U8, torch.int16: _lib.const.PIX_U16, torch.float32: _lib.const.PIX_F32,
        torch.float64: _lib.const.PIX_F64}      # (int16: the bits of a uint16 frame where torch has no uint16)
if hasattr(torch, 'uint16'):
    _PIX[torch.uint16] = _lib.const.PIX_U16


def _prestep(cubic_map, raw, dst, dst_frame_stride):
    """one camera: raw frames [n,h,w] / [n,h,w,3] -> u8 grey frames at dst.data_ptr() + f * dst_frame_stride"""
    h, w = cubic_map.shape[:2]
    with torch.cuda.device(cubic_map.device):
        _lib.check(_lib.load().cpe_matlab_prestep_batch(raw.data_ptr(), raw.shape[0], h, w, _PIX[raw.dtype], 3 if raw.dim() == 4 else 1,
                                                        cubic_map.data_ptr(), 0, dst.data_ptr(), dst_frame_stride,
                                                        torch.cuda.current_stream().cuda_stream), 'cpe_matlab_prestep_batch')


class StereoPrestep:
    """utils/preProcessing.m:3-9 for chunks of stereo frames, resident on the GPU: im2uint8 + undistortImage(..., 'cubic') +
    rgb2gray of both cameras in one kernel per camera (cpe_matlab_prestep_batch), written as frame-major pairs [F,2,h,w]:
    the layout FramePipeline reads in place.  The two MATLAB maps are built once.

    Raw frames are device tensors [F,h,w] or [F,h,w,3] (RGB, channel-last) of dtype uint8, uint16, float32 or float64; an
    int16 tensor is taken as the uint16 bit pattern.  The two cameras may differ in dtype and channels."""

    def __init__(self, cam_left, cam_right, h, w, device='cuda:0'):
        self.h, self.w = int(h), int(w)
        self.maps = tuple(Undistorter(cam, h, w, device, interp='cubic').map for cam in (cam_left, cam_right))
        self.device = self.maps[0].device           # with its index: 'cuda' names the device the maps were made on

    def _check(self, raw, what):
        if raw.device != self.device:
            raise _lib.CpeError(f'StereoPrestep: {what} frames are on {raw.device}, the maps on {self.device}')
        if not raw.is_contiguous() or raw.dtype not in _PIX or raw.dim() not in (3, 4) \
                or tuple(raw.shape[1:3]) != (self.h, self.w) or (raw.dim() == 4 and raw.shape[3] != 3):
            raise _lib.CpeError(f'StereoPrestep: {what} frames must be contiguous [F,{self.h},{self.w}] or [F,{self.h},{self.w},3] '
                                f'of uint8, uint16 (or int16 bits), float32 or float64')

    def __call__(self, left_raw, right_raw, out=None):
        """-> u8 [F,2,h,w] (out[:, 0] left, out[:, 1] right): two launches on the current stream, no host synchronisation"""
        self._check(left_raw, 'left'); self._check(right_raw, 'right')
        F = left_raw.shape[0]
        if right_raw.shape[0] != F:
            raise _lib.CpeError('StereoPrestep: left and right differ in frame count')
        if out is None:
            out = torch.empty((F, 2, self.h, self.w), dtype=torch.uint8, device=self.device)
        elif out.dtype != torch.uint8 or tuple(out.shape) != (F, 2, self.h, self.w) or not out.is_contiguous() or out.device != self.device:
            raise _lib.CpeError(f'StereoPrestep: out must be contiguous u8 [{F},2,{self.h},{self.w}] on {self.device}')
        N = self.h * self.w
        _prestep(self.maps[0], left_raw, out[:, 0], 2 * N)
        _prestep(self.maps[1], right_raw, out[:, 1], 2 * N)
        return out


def _raw_image(image, what):
    img = np.array(image, copy=True, order='C')     # (PIL / MATLAB hand over read-only buffers)
    if img.dtype.name not in ('uint8', 'uint16', 'float32', 'float64') or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] < 3):
        raise _lib.CpeError(f'preprocessing: {what} image must be [h,w] or [h,w,3] of uint8, uint16, float32 or float64')
    if img.ndim == 3 and img.shape[2] > 3:
        img = np.ascontiguousarray(img[..., :3])    # (further planes, such as alpha, are not part of the grey value)
    return torch.from_numpy(img.view(np.int16) if img.dtype == np.uint16 else img)[None]


def preprocessing(input_img_l, input_img_r, camera_params_l, camera_params_r, device='cuda:0'):
    """utils/preProcessing.m: im2uint8 + undistortImage(..., 'cubic') + rgb2gray for both cameras -> (imgL_uint8, imgR_uint8).
    (Its third and fourth outputs, adapthisteq pictures, feed nothing on the detection path: exp_gridDetection.m:67-68 hands
    the undistorted images to makePyGridPts.)  Colour input is converted AFTER the undistortion, as in the .m file.
    Images are numpy [h,w] or [h,w,3] (RGB) of uint8, uint16, float32 or float64, as imread hands them to im2uint8; the two
    may differ in size.  Of an image with more than 3 planes the first three are taken as R, G, B.
    Per camera: one upload, one kernel (StereoPrestep's), one download."""
    out = []
    for what, img, cam in (('left', input_img_l, camera_params_l), ('right', input_img_r, camera_params_r)):
        raw = _raw_image(img, what)
        h, w = raw.shape[1:3]
        und = Undistorter(cam, h, w, device, 'cubic')
        dst = torch.empty((1, h, w), dtype=torch.uint8, device=und.device)
        _prestep(und.map, raw.to(und.device), dst, h * w)
        out.append(dst[0].cpu().numpy())
    return out[0], out[1]
