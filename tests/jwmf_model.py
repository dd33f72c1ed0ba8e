"""CPU model of psm_joint_wmf: the joint weighted median of the reference's PP::processDM
(src/PP.cpp:417-422 -> JointWMF::filter, include/JointWMF.h), with the semantics DESIGN.md section 9 pins down:

  feature   the 8-bit colour image (JointWMF.h convertTo(CV_8UC3, 255) of a float image: saturate(rint(v*255)))
  keys      6-bit (c0>>2, c1>>2, c2>>2) per pixel, c0 = the first interleaved channel (B)  (JointWMF.h:546-567)
  samples   the distinct keys, ascending                                                    (JointWMF.h:575-582)
  clusters  identity when there are at most n_clusters samples; otherwise k-means++ seeding from a fixed splitmix64
            stream and Lloyd iterations in fp32 (the reference's cv::kmeans draws from an unreproducible RNG state)
  table     w[i][j] = expf(-((d0*d0 + d1*d1) + d2*d2) * divider) over the centres          (JointWMF.h:615-645)
  median    smallest c in [0, 255] with 2 * W(<=c) >= W(total) over the clipped window, the weights summed as the
            exact integers rint(w * 2^48)                                                   (JointWMF.h:272-315)
"""
from __future__ import annotations

import ctypes
import ctypes.util
import os

import numpy as np

M64 = (1 << 64) - 1
SEED = 0x4A574D46          # splitmix64 state the k-means++ seeding starts from (the library's JW_SEED)
WQ_SCALE = 2.0 ** 48


class SplitMix64:
    def __init__(self, seed: int = SEED):
        self.s = seed & M64

    def next(self) -> int:
        self.s = (self.s + 0x9E3779B97F4A7C15) & M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)


def feature_u8(img) -> np.ndarray:
    """H x W x 3 feature bytes: uint8 images as they are, float images saturate(rint(v * 255.0f))."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img
    f = np.rint(img.astype(np.float32) * np.float32(255.0))
    return np.where(f > 0, np.minimum(f, np.float32(255)), np.float32(0)).astype(np.uint8)   # (NaN -> 0)


def keys_of(feat: np.ndarray) -> np.ndarray:
    f = feat.astype(np.int32) >> 2
    return (f[..., 0] << 12) | (f[..., 1] << 6) | f[..., 2]


def key_xyz(keys: np.ndarray) -> np.ndarray:
    keys = np.asarray(keys, np.int64)
    return np.stack([keys >> 12, (keys >> 6) & 63, keys & 63], axis=-1)


def _assign(xyz_f: np.ndarray, centres: np.ndarray) -> np.ndarray:
    """Nearest centre, distance ((t0*t0 + t1*t1) + t2*t2) in fp32, ties to the lower index (argmin takes the first)."""
    out = np.empty(len(xyz_f), np.int64)
    for a in range(0, len(xyz_f), 16384):
        t = xyz_f[a:a + 16384, None, :] - centres[None, :, :]
        d = (t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2]
        out[a:a + 16384] = np.argmin(d, axis=1)
    return out


def cluster(samples: np.ndarray, n_clusters: int = 256, max_iter: int = 10000):
    """samples: ascending distinct keys.  -> (labels per sample, centres [nF, 3] float32, iterations)."""
    xyz = key_xyz(samples)
    n = len(samples)
    if n <= n_clusters:                                   # every key its own cluster (the reference's result for any RNG state)
        return np.arange(n, dtype=np.int64), xyz.astype(np.float32), 0
    nf = n_clusters
    rng = SplitMix64()
    seeds = [rng.next() % n]
    d2 = ((xyz - xyz[seeds[0]]) ** 2).sum(axis=1)
    for _ in range(1, nf):
        pref = np.cumsum(d2)
        r = rng.next() % int(pref[-1])
        j = int(np.searchsorted(pref, r, side="right"))   # first sample whose inclusive prefix exceeds r
        seeds.append(j)
        d2 = np.minimum(d2, ((xyz - xyz[j]) ** 2).sum(axis=1))
    centres = xyz[seeds].astype(np.float32)
    xyz_f = xyz.astype(np.float32)
    labels = np.full(n, -1, np.int64)
    it = max_iter
    for k in range(1, max_iter + 1):
        new = _assign(xyz_f, centres)
        changed = int(np.count_nonzero(new != labels))
        labels = new
        if changed == 0:
            it = k
            break
        cnt = np.bincount(labels, minlength=nf)
        for c in range(3):
            s = np.bincount(labels, weights=xyz[:, c], minlength=nf).astype(np.int64)
            upd = (s.astype(np.float32) / cnt.astype(np.float32)).astype(np.float32)
            centres[:, c] = np.where(cnt > 0, upd, centres[:, c])
    return labels, centres, it


def label_of_key(samples: np.ndarray, labels: np.ndarray) -> np.ndarray:
    lok = np.zeros(64 ** 3, np.uint8)
    lok[samples] = labels
    return lok


_libm = None


def expf(x: float) -> float:
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m"))
        _libm.expf.restype = ctypes.c_float
        _libm.expf.argtypes = [ctypes.c_float]
    return _libm.expf(x)


def weight_table(centres: np.ndarray, sigma: float = 25.5) -> np.ndarray:
    """[nF, nF] float32, JointWMF.h:615-645 ("exp"): nSigmaI = sigma/256.0f*64, divider = 1.0f/(2*nSigmaI*nSigmaI)."""
    f32 = np.float32
    ns = f32(f32(sigma) / f32(256.0)) * f32(64)
    divider = f32(1.0) / f32(f32(2) * ns * ns)
    c = np.asarray(centres, np.float32)
    t = c[:, None, :] - c[None, :, :]
    s = (t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2]
    arg = (-s) * divider
    uniq, inv = np.unique(arg, return_inverse=True)
    vals = np.array([expf(float(a)) for a in uniq], np.float32)
    return vals[inv].reshape(arg.shape)


def quantise(w: np.ndarray) -> np.ndarray:
    return np.rint(np.asarray(w, np.float32).astype(np.float64) * WQ_SCALE).astype(np.int64)


def median(dmap: np.ndarray, F: np.ndarray, wq: np.ndarray, r: int, pixels=None) -> np.ndarray:
    """Joint weighted median of the u8 map `dmap` with label plane F and integer table wq.  pixels: optional (ys, xs) to
    evaluate only those (the rest keep the input value)."""
    H, W = dmap.shape
    out = dmap.copy()
    if pixels is None:
        ys, xs = np.divmod(np.arange(H * W), W)
    else:
        ys, xs = np.asarray(pixels[0]), np.asarray(pixels[1])
    dy, dx = np.mgrid[-r:r + 1, -r:r + 1]
    dy, dx = dy.ravel(), dx.ravel()
    d = dmap.astype(np.int64)
    for a in range(0, len(ys), 4096):
        y, x = ys[a:a + 4096], xs[a:a + 4096]
        qy, qx = y[:, None] + dy[None, :], x[:, None] + dx[None, :]
        ok = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
        qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
        dq = d[qy, qx]
        w = np.where(ok, wq[F[y, x][:, None], F[qy, qx]], 0)
        order = np.argsort(dq, axis=1, kind="stable")
        dq = np.take_along_axis(dq, order, 1)
        cum = np.cumsum(np.take_along_axis(w, order, 1), axis=1)
        j = np.argmax(2 * cum >= cum[:, -1:], axis=1)
        out[y, x] = dq[np.arange(len(y)), j]
    return out


def clustering_of(img, n_clusters: int = 256, max_iter: int = 10000):
    """-> dict(samples, labels, centres, iterations, lok, F) for one image."""
    keys = keys_of(feature_u8(img))
    samples = np.unique(keys)
    labels, centres, it = cluster(samples, n_clusters, max_iter)
    lok = label_of_key(samples, labels)
    return {"samples": samples, "labels": labels, "centres": centres, "iterations": it, "lok": lok, "F": lok[keys]}


def joint_wmf(dmap, img, r: int = 9, sigma: float = 25.5, n_clusters: int = 256, max_iter: int = 10000,
              clusters=None, pixels=None):
    """One map through the whole filter.  clusters: (centres, lok) to use instead of the default clustering."""
    if clusters is None:
        cl = clustering_of(img, n_clusters, max_iter)
        centres, F = cl["centres"], cl["F"]
    else:
        centres, lok = clusters
        F = np.asarray(lok)[keys_of(feature_u8(img))]
    wq = quantise(weight_table(centres, sigma))
    return median(np.asarray(dmap, np.uint8), F, wq, r, pixels)


def brute_median(dmap, F, wq, r: int):
    """The definition in Python integers, pixel by pixel (tiny images only)."""
    H, W = dmap.shape
    out = np.zeros_like(dmap)
    for y in range(H):
        for x in range(W):
            taps = [(int(dmap[qy, qx]), int(wq[F[y, x], F[qy, qx]]))
                    for qy in range(max(0, y - r), min(H - 1, y + r) + 1)
                    for qx in range(max(0, x - r), min(W - 1, x + r) + 1)]
            tot = sum(w for _, w in taps)
            for c in range(256):
                if 2 * sum(w for dv, w in taps if dv <= c) >= tot:
                    out[y, x] = c
                    break
    return out


def load_reading(build_dir: str):
    """Compile tests/jwmf_reading.c (the serial restatement of the reference's filterCore) and bind it with ctypes."""
    import subprocess
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jwmf_reading.c")
    so = os.path.join(build_dir, "jwmf_reading.so")
    subprocess.run(["cc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", so, "-lm"], check=True)
    lib = ctypes.CDLL(so)
    P = ctypes.c_void_p
    lib.jwmf_reading_core.argtypes = [P, P, P] + [ctypes.c_int] * 5 + [P]
    lib.jwmf_reading_identity.argtypes = [P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, P]
    return lib


def reading_core(lib, dmap, F, w, r: int) -> np.ndarray:
    """The reading's column scan with the float table w [nF, nF] and cluster plane F."""
    H, W = dmap.shape
    I = np.ascontiguousarray(dmap, np.int32)
    Fi = np.ascontiguousarray(F, np.int32)
    wt = np.ascontiguousarray(w, np.float32)
    out = np.zeros((H, W), np.int32)
    assert lib.jwmf_reading_core(I.ctypes.data, Fi.ctypes.data, wt.ctypes.data, wt.shape[0], 256, H, W, r, out.ctypes.data) == 0
    return out.astype(np.uint8)


def reading_identity(lib, img, dmap, r: int = 9, sigma: float = 25.5):
    """The reading of the whole filter for a u8 image with at most 256 distinct keys -> (map, nF)."""
    H, W = dmap.shape
    im = np.ascontiguousarray(img, np.uint8)
    dm = np.ascontiguousarray(dmap, np.uint8)
    out = np.zeros((H, W), np.uint8)
    nf = lib.jwmf_reading_identity(im.ctypes.data, dm.ctypes.data, H, W, r, sigma, out.ctypes.data)
    return out, nf


def near_tie(dmap, F, w, r: int, y: int, x: int, a: int, b: int, tol: float = 1e-3) -> bool:
    """Some c between a and b has |W(<=c) - W(>c)| < tol, W summed in fp64 from the float table (the rule's float walk can
    land on either side of such a c)."""
    H, W = dmap.shape
    ys, xs = slice(max(0, y - r), min(H - 1, y + r) + 1), slice(max(0, x - r), min(W - 1, x + r) + 1)
    d = dmap[ys, xs].ravel().astype(np.int64)
    wt = np.asarray(w, np.float64)[F[y, x], F[ys, xs].ravel()]
    tot = wt.sum()
    for c in range(min(a, b), max(a, b) + 1):
        le = wt[d <= c].sum()
        if abs(le - (tot - le)) < tol:
            return True
    return False
