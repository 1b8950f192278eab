"""Row f-3: time the fused pre-step (iotool.StereoPrestep: im2uint8 + cubic undistortion + rgb2gray, one kernel per camera,
written as frame-major pairs) against the same result from the separate calls, for every element type and channel count.

    python tools/time_prestep.py [--pairs 64] [--reps 12] [--procs 3] [--child-timeout 300] [--out FILE]

Variants, timed by the protocol of tools/timing.py between device events:
    a   StereoPrestep into an [F,2,h,w] tensor
    b   torch im2uint8 -> Undistorter(cubic) over the planes -> torch-f64 grey expression -> copy into the pairs tensor
a and b must give equal bytes before anything is timed.  The summary of a case carries b's run-to-run spread.
Also: wall time per pair of the one-image-at-a-time host path (upload, remap per plane, download, upload, torch grey,
download) that iotool.preprocessing was before the fused kernel, for u8 grey and u8 RGB host arrays."""
import argparse
import json
import sys
import time

import timing

H, W = 1200, 1920
CAMS = [dict(IntrinsicMatrix=[[1400.0, 0.3, 955.5], [0, 1398.0, 601.25], [0, 0, 1]], RadialDistortion=[-0.21, 0.07], TangentialDistortion=[0.001, -0.0007]),
        dict(IntrinsicMatrix=[[1402.0, 0.2, 963.0], [0, 1401.0, 598.75], [0, 0, 1]], RadialDistortion=[-0.20, 0.06], TangentialDistortion=[-0.0006, 0.0009])]
CASES = [(dt, ch) for dt in ('uint8', 'uint16', 'float32', 'float64') for ch in (1, 3)]
ESIZE = dict(uint8=1, uint16=2, float32=4, float64=8)
REMAP_FRAMES = 8                 # csrc/undistort.hip: frames per map read
HBM_PEAK = 8e12                  # bytes/s


def algorithmic_bytes_per_pixel(dtype, ch):
    """per output pixel of one frame: the source elements, the byte written, the 8 B map entry once per frame group"""
    return ESIZE[dtype] * ch + 1 + 8.0 / REMAP_FRAMES


def child(pairs, reps):
    import numpy as np
    import torch
    import cpe_amd  # noqa: F401
    from cpe_amd import iotool
    dev = torch.device('cuda:0')
    pre = iotool.StereoPrestep(CAMS[0], CAMS[1], H, W, dev)
    unds = [iotool.Undistorter(c, H, W, dev, interp='cubic') for c in CAMS]

    def raw(dtype, ch, seed):
        g = torch.Generator(device=dev); g.manual_seed(seed)
        shape = (pairs, H, W) + ((3,) if ch == 3 else ())
        if dtype == 'uint8':
            return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)
        if dtype == 'uint16':
            return (torch.randint(0, 65536, shape, dtype=torch.int32, device=dev, generator=g)).to(torch.int16)   # uint16 bits
        return torch.rand(shape, dtype=getattr(torch, dtype), device=dev, generator=g) * 1.1 - 0.05

    def im2uint8(x):
        if x.dtype == torch.uint8:
            return x
        if x.dtype == torch.int16:
            return (((x.to(torch.int32) & 0xFFFF) + 128) // 257).to(torch.uint8)
        v = x * 255
        f = torch.floor(v)
        r = f + (v - f >= 0.5).to(v.dtype)                   # half away from zero on the exact value
        return torch.nan_to_num(r, nan=0.0).clamp_(0, 255).to(torch.uint8)

    def separate(x, und, dst):
        u = im2uint8(x)
        if u.dim() == 3:
            dst.copy_(und(u))
            return
        n = u.shape[0]
        t = und(u.permute(0, 3, 1, 2).reshape(3 * n, H, W).contiguous()).reshape(n, 3, H, W).to(torch.float64)
        g = t[:, 0] * 0.298936021293775 + t[:, 1] * 0.587043074451121 + t[:, 2] * 0.114020904255103
        dst.copy_(torch.floor(g + 0.5).clamp_(0, 255).to(torch.uint8))

    out_a = torch.empty((pairs, 2, H, W), dtype=torch.uint8, device=dev)
    out_b = torch.empty_like(out_a)
    for dtype, ch in CASES:
        L, R = raw(dtype, ch, 1), raw(dtype, ch, 2)
        variants = dict(a=lambda: pre(L, R, out=out_a),
                        b=lambda: (separate(L, unds[0], out_b[:, 0]), separate(R, unds[1], out_b[:, 1])))
        for f in variants.values():                          # warm-up, and the equality that makes the timing meaningful
            f(); f()
        torch.cuda.synchronize()
        assert torch.equal(out_a, out_b), f'{dtype} x{ch}: fused and separate results differ'
        ms = timing.event_loop(variants, reps)
        print(json.dumps(dict(kind='case', dtype=dtype, channels=ch, pairs=pairs, reps=reps, median_ms=timing.medians(ms), ms=ms)), flush=True)
        del L, R, variants
        torch.cuda.empty_cache()
    # the one-image-at-a-time host path: per plane upload + remap + download, then upload + torch-f64 grey + download
    rng = np.random.default_rng(0)
    for ch in (1, 3):
        imgs = [rng.integers(0, 256, (H, W) + ((3,) if ch == 3 else ()), dtype=np.uint8) for _ in range(2)]

        def one_pair():
            for img, cam in zip(imgs, CAMS):
                u = iotool.undistort_image(img, cam, dev, 'cubic')
                if u.ndim == 3:
                    t = torch.from_numpy(u).to(dev).to(torch.float64)
                    g = t[..., 0] * 0.298936021293775 + t[..., 1] * 0.587043074451121 + t[..., 2] * 0.114020904255103
                    u = torch.floor(g + 0.5).clamp_(0, 255).to(torch.uint8).cpu().numpy()
        one_pair()
        t0 = time.perf_counter()
        for _ in range(5):
            one_pair()
        host = (time.perf_counter() - t0) / 5
        t0 = time.perf_counter()
        for _ in range(5):
            iotool.preprocessing(imgs[0], imgs[1], CAMS[0], CAMS[1], dev)
        now = (time.perf_counter() - t0) / 5
        print(json.dumps(dict(kind='host', channels=ch, separate_ms_per_pair=host * 1e3, preprocessing_ms_per_pair=now * 1e3)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=64)
    a = timing.parse(ap, reps=12, child_timeout=300.0)      # a child is 8 cases + the host path
    if a.child:
        return child(a.pairs, a.reps)
    lines, emit = timing.run_children(__file__, a)
    for dtype, ch in CASES:
        rows = [d for d in lines if d['kind'] == 'case' and d['dtype'] == dtype and d['channels'] == ch]
        med, spreads = timing.reduce(rows)
        spread = spreads['b']
        bpp = algorithmic_bytes_per_pixel(dtype, ch)
        rate = bpp * 2 * a.pairs * H * W / (med['a'] * 1e-3)
        verdict = med['a'] <= med['b'] + spread
        d = dict(kind='summary', dtype=dtype, channels=ch, pairs=a.pairs, fused_ms=med['a'], separate_ms=med['b'],
                 separate_spread_ms=spread, fused_not_slower=verdict, algorithmic_bytes_per_pixel=bpp, algorithmic_GBps=rate / 1e9,
                 share_of_8TBps_hbm_peak=rate / HBM_PEAK)
        emit(d)
    return 0


if __name__ == '__main__':
    sys.exit(main())
