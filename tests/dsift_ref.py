"""Test oracle of the dense-SIFT producer (test helper; numpy / torch CPU only, never imported by the product).

Two independent float64 restatements of the descriptor defined in DESIGN.md §16 (the reference's `dsift` model,
pixsfm/features/models/dsift.py: kornia's DenseSIFTDescriptor(num_ang_bins=8, num_spatial_bins=4, spatial_bin_size=s,
rootsift, clipval, stride=1, padding=1) on the grey image):
  dsift_numpy  slices of numpy arrays written from the formulas;
  dsift_torch  the way kornia composes it: F.pad(replicate) + conv2d for the gradient, conv2d with the outer-product pooling
               kernel and padding s/2, conv2d with eye(128).view(128, 8, 4, 4) and padding 1, F.normalize.
kornia itself is not available here: the definition is "parity unpinned (kornia absent)".
Plus the host side of FeatureExtractor (extractor.py:152-199): L2 normalisation, cast, corners, the ps x ps gather.
"""
import math

import numpy as np

EPS = 1e-10


def pool_kernel(s):
    """k(i) = (s/2 - |i + 0.5 - s/2|) / (s/2), i = 0 .. s-1 (kornia get_sift_pooling_kernel, separated)."""
    hs = s / 2.0
    return np.array([(hs - abs(i + 0.5 - hs)) / hs for i in range(s)])


def _normalise(D, rootsift, clipval):
    """Step 5 over axis 0 (the 128 channels)."""
    n = D / np.maximum(np.sqrt((D * D).sum(0)), 1e-12)
    n = np.clip(n, 0.0, clipval)
    n = n / np.maximum(np.sqrt((n * n).sum(0)), 1e-12)
    if rootsift:
        n = np.sqrt(n / np.maximum(np.abs(n).sum(0), 1e-12) + EPS)
    return n


def dsift_numpy(img, spatial_bin_size=4, rootsift=True, clipval=0.2):
    """(h, w) grey image (float values) -> (128, h, w) float64."""
    s = int(spatial_bin_size)
    I = np.asarray(img, dtype=np.float64)
    h, w = I.shape
    Ip = np.pad(I, 1, mode="edge")                                  # indices clamped into the image
    gx = 0.5 * Ip[1:-1, 2:] - 0.5 * Ip[1:-1, :-2]
    gy = 0.5 * Ip[2:, 1:-1] - 0.5 * Ip[:-2, 1:-1]
    mag = np.sqrt(gx * gx + gy * gy + EPS)
    o = 8.0 * (np.arctan2(gy, gx + EPS) + 2 * math.pi) / (2 * math.pi)
    f = np.floor(o)
    w1 = o - f
    b0 = np.mod(f, 8).astype(np.int64)
    b1 = (b0 + 1) % 8
    A = np.zeros((8, h, w))
    for a in range(8):
        A[a] = np.where(b0 == a, (1.0 - w1) * mag, 0.0) + np.where(b1 == a, w1 * mag, 0.0)
    # P_a(j, i) = sum_{u,v} k(u) k(v) A_a(j + u - s/2, i + v - s/2), A zero outside the image, 0 <= j <= h, 0 <= i <= w
    k = pool_kernel(s)
    Ap = np.zeros((8, h + s, w + s))
    Ap[:, s // 2:s // 2 + h, s // 2:s // 2 + w] = A
    P = np.zeros((8, h + 1, w + 1))
    for u in range(s):
        for v in range(s):
            P += k[u] * k[v] * Ap[:, u:u + h + 1, v:v + w + 1]
    # D_c(y, x) = P_a(y + sy - 1, x + sx - 1), c = 16 a + 4 sy + sx, P zero outside [0, h] x [0, w]
    Pp = np.zeros((8, h + 3, w + 3))
    Pp[:, 1:h + 2, 1:w + 2] = P
    D = np.zeros((128, h, w))
    for a in range(8):
        for sy in range(4):
            for sx in range(4):
                D[16 * a + 4 * sy + sx] = Pp[a, sy:sy + h, sx:sx + w]
    return _normalise(D, rootsift, clipval)


def dsift_torch(img, spatial_bin_size=4, rootsift=True, clipval=0.2, dtype=np.float64):
    """The same as a torch CPU composition of convolutions (kornia's structure) -> (128, h, w) numpy array of `dtype`
    (float64: the oracle; float32: the reference model's own arithmetic)."""
    import torch
    import torch.nn.functional as F
    s = int(spatial_bin_size)
    tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    x = torch.as_tensor(np.asarray(img, dtype=dtype))[None, None]
    h, w = x.shape[2:]
    xp = F.pad(x, (1, 1, 1, 1), mode="replicate")
    kx = torch.tensor([[0.0, 0.0, 0.0], [-0.5, 0.0, 0.5], [0.0, 0.0, 0.0]], dtype=tdt)
    gx = F.conv2d(xp, kx[None, None])
    gy = F.conv2d(xp, kx.t().contiguous()[None, None])
    mag = torch.sqrt(gx * gx + gy * gy + EPS)
    o = 8.0 * (torch.atan2(gy, gx + EPS) + 2.0 * math.pi) / (2.0 * math.pi)
    f = torch.floor(o)
    w1 = o - f
    b0 = torch.remainder(f, 8)
    b1 = torch.remainder(b0 + 1, 8)
    A = torch.cat([(b0 == a).to(tdt) * (1.0 - w1) * mag + (b1 == a).to(tdt) * w1 * mag for a in range(8)], 1)
    k = torch.as_tensor(pool_kernel(s), dtype=tdt)
    pool = torch.outer(k, k)[None, None]
    P = F.conv2d(A.view(8, 1, h, w), pool, padding=s // 2).view(1, 8, h + 1, w + 1)
    gather = torch.eye(128, dtype=tdt).view(128, 8, 4, 4)
    D = F.conv2d(P, gather, padding=1)
    out = F.normalize(D, dim=1, p=2).clamp(0.0, float(clipval))
    out = F.normalize(out, dim=1, p=2)
    if rootsift:
        out = torch.sqrt(F.normalize(out, dim=1, p=1) + EPS)
    return out[0].numpy()


def grey_of(image):
    """PIL image / uint8 array -> the grey values the model sees: PIL convert("L"), to_tensor (value / 255 in float32)."""
    from PIL import Image
    if not isinstance(image, Image.Image):
        image = Image.fromarray(np.asarray(image))
    u8 = np.asarray(image.convert("L"))
    return u8, u8.astype(np.float32) / np.float32(255.0)


def corners_of(keypoints, scale, ps, h, w):
    """extractor.py:192-193: clip(int(kp * scale - ps / 2), 0, (w, h) - ps - 1)."""
    c = (np.asarray(keypoints, dtype=np.float64).reshape(-1, 2) * scale - ps / 2.0).astype(np.int32)
    return np.clip(c, [0, 0], np.array([w, h]) - ps - 1)


def sparse_patches(fmap, keypoints, image_size, ps=16, l2_normalize=True, dtype=np.float16):
    """The sparse branch of tensor_to_fmap on a (C, h, w) map: L2 normalisation in fp32, cast, corners, (n, ps, ps, C)."""
    fm = np.asarray(fmap, dtype=np.float32)
    C, h, w = fm.shape
    if l2_normalize:
        fm = fm / np.maximum(np.sqrt((fm.astype(np.float64) ** 2).sum(0)), 1e-12).astype(np.float32)
    fm = fm.astype(dtype)
    scale = np.array((w / image_size[0], h / image_size[1]))
    corners = corners_of(keypoints, scale, ps, h, w)
    hwc = fm.transpose(1, 2, 0)
    patches = np.stack([hwc[y:y + ps, x:x + ps] for x, y in corners]) if len(corners) else np.zeros((0, ps, ps, C), dtype)
    return patches, corners, scale
