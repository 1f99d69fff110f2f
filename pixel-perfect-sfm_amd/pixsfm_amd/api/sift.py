"""SIFT keypoints and descriptors for the accelerated path: photographs -> what the matcher and the extractor take.

The reference is started from hloc's `extract_features` with the `sift` configuration or from a COLMAP SIFT database; neither
pycolmap, VLFeat nor OpenCV is installable where this library runs, so the stage is native here (pxr_sift_*, DESIGN.md section
25).  `SiftExtractor.create(conf).extract_images(image_dir, names)` returns `({name: keypoints}, {name: descriptors})`: the first
is what `features_from_image_list` takes, the second what `DescriptorMatcher.match_pairs` takes.  The kernels reproduce bit for
bit; parity with VLFeat / COLMAP is not pinned.

Keypoints are returned in COLMAP's convention, as everywhere in this package (the centre of the top-left pixel is (0.5, 0.5));
the C-ABI below works in pixel indices.
"""
import os

import numpy as np

from ..engine import SiftPyramid, sift_options
from . import base
from .keypoint_adjustment import default_context


class SiftExtractor:
    """SIFT detection and description of grey images -- in place of hloc.extract_features(conf "sift")."""
    default_conf = {
        'first_octave': -1,            # -1: start from the doubled image (hloc's and COLMAP's default); 0: from the image
        'num_octaves': 0,              # 0: automatic
        'octave_resolution': 3,
        'sigma0': 1.6,
        'sigma_in': 0.5,
        'peak_threshold': None,        # None: 0.02 / octave_resolution
        'edge_threshold': 10.0,
        'max_refine_steps': 5,
        'max_num_orientations': 2,
        'upright': False,
        'normalization': 'L1_ROOT',    # 'L1_ROOT' ("rootsift") or 'L2'
        'magnif': 3.0,
        'clip': 0.2,
        'max_num_features': None,      # keep the largest scales (ties by order), as COLMAP does; None: all
        'device': False,               # True: return device arrays and copy nothing to the host
    }
    _NORMALIZATIONS = {'L2': 0, 'L1_ROOT': 1}

    def __init__(self, conf=None, ctx=None):
        self.conf = base.merge_conf(self.default_conf, conf)
        if self.conf['normalization'] not in self._NORMALIZATIONS:
            raise ValueError("normalization must be 'L2' or 'L1_ROOT' (got %r)" % (self.conf['normalization'],))
        m = self.conf['max_num_features']
        if m is not None and int(m) < 0:
            raise ValueError("max_num_features must not be negative")
        sift_options(**self.options())                     # (a value of the wrong type fails here, not at the first image)
        self.ctx = ctx
        self.kernel_ms = {}

    @classmethod
    def create(cls, conf=None, ctx=None):
        """conf: a dict over default_conf; an unknown key is a ValueError."""
        return cls(conf, ctx)

    def options(self):
        """The keyword arguments of engine.sift_options."""
        c = self.conf
        o = {k: c[k] for k in ('first_octave', 'num_octaves', 'octave_resolution', 'sigma0', 'sigma_in', 'edge_threshold',
                               'max_refine_steps', 'max_num_orientations', 'magnif', 'clip')}
        o['peak_threshold'] = -1.0 if c['peak_threshold'] is None else c['peak_threshold']
        o['upright'] = int(bool(c['upright']))
        o['normalization'] = self._NORMALIZATIONS[c['normalization']]
        return o

    @staticmethod
    def _grey(image):
        """A path, a PIL image, or an (h, w) / (h, w, 3) uint8 or float32 array -> (h, w) uint8 or float32 (PIL convert("L"))."""
        if isinstance(image, (str, bytes)) or hasattr(image, "__fspath__"):
            from PIL import Image
            with Image.open(image) as im:
                return np.ascontiguousarray(np.asarray(im.convert("L")))
        if hasattr(image, "convert"):
            return np.ascontiguousarray(np.asarray(image.convert("L")))
        if getattr(image, "__cuda_array_interface__", None) is not None:
            return image
        a = np.asarray(image)
        if a.ndim == 3 and a.shape[2] == 3 and a.dtype == np.uint8:
            from PIL import Image
            a = np.asarray(Image.fromarray(a).convert("L"))
        if a.ndim != 2 or a.dtype not in (np.uint8, np.float32):
            raise ValueError("image must be (h, w) uint8 or float32, or (h, w, 3) uint8 (got %s %s)" % (a.shape, a.dtype))
        return np.ascontiguousarray(a)

    def _pyramid(self, image, timed):
        return SiftPyramid(self.ctx or default_context(), self._grey(image), timed=timed, **self.options())

    def extract(self, image, timed=False):
        """image -> {"keypoints" (n, 2) COLMAP coordinates, "scales" (n,), "orientations" (n,), "scores" (n,), "descriptors"
        (n, 128) float32}: host arrays, or with conf device=True device arrays.  Features are in the detector's order (octave,
        level, row, column, rank of the orientation); with max_num_features the largest scales are kept, in that order."""
        pyr = self._pyramid(image, timed)
        kp, _, resp, _ = pyr.detect(timed=timed)
        index = None
        m = self.conf['max_num_features']
        if m is not None and kp.shape[0] > int(m):
            sigma = kp.download()[:, 2]
            index = np.sort(np.argsort(-sigma, kind="stable")[:int(m)])
        kp4, xy, scales, orient, scores = pyr.gather(kp, resp, index, offset=0.5)
        desc, _ = pyr.describe(kp4, timed=timed)
        self.kernel_ms = dict(pyr.kernel_ms)
        out = dict(keypoints=xy, scales=scales, orientations=orient, scores=scores, descriptors=desc)
        return out if self.conf['device'] else {k: v.download() for k, v in out.items()}

    def describe(self, image, keypoints, scales, orientations, timed=False):
        """Descriptors (n, 128) float32 and their validity (n,) bool for given keypoints (COLMAP coordinates), scales and
        orientations -- keypoints that keypoint adjustment moved, say.  Host arrays, or device arrays with conf device=True."""
        kp = np.asarray(keypoints, dtype=np.float64).reshape(-1, 2) - 0.5
        rows = np.column_stack([kp, np.asarray(scales, dtype=np.float64).reshape(-1), np.asarray(orientations, dtype=np.float64).reshape(-1)])
        pyr = self._pyramid(image, timed)
        desc, valid = pyr.describe(rows, timed=timed)
        self.kernel_ms = dict(pyr.kernel_ms)
        return (desc, valid) if self.conf['device'] else (desc.download(), valid.download().astype(bool))

    def extract_images(self, image_dir, names):
        """-> ({name: keypoints (n, 2)}, {name: descriptors (n, 128)}): what features_from_image_list and
        DescriptorMatcher.match_pairs take."""
        keypoints, descriptors = {}, {}
        for name in names:
            r = self.extract(os.path.join(str(image_dir), name))
            keypoints[name], descriptors[name] = r["keypoints"], r["descriptors"]
        return keypoints, descriptors
