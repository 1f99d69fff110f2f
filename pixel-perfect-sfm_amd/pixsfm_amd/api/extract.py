"""Dense feature extraction from images: pixsfm.features.FeatureExtractor and pixsfm.extract.features_from_image_list /
features_from_graph / features_from_reconstruction (pixsfm/features/extractor.py, pixsfm/extract.py) for the weight-free
models, on the GPU.

  "dsift"  the reference's dense SIFT (pixsfm/features/models/dsift.py, pixsfm/configs/dsift.yaml): HIP kernels
           (csrc/pxr_dsift.hip).  Sparse extraction computes the descriptors only on the patch windows and writes them
           straight into a patch arena (pxr_dsift_extract); the dense branch runs the dense kernel (pxr_dsift_dense).
  "image"  the reference's `image` model (features/models/image.py): RGB (or grey) / 255, patches by pxr_arena_extract.
The learned models (s2dnet, vggnet) need weights and stay in PyTorch: ValueError.  The host side -- image
decoding, the max_edge / pyr_scales resize, the grey conversion -- is PIL, as in the reference.  There is no CPU path.
"""
import copy
import os
import re
from collections import OrderedDict

import numpy as np

from .features import FeatureManager, FeatureMap, fmap_from_arena, kDenseId

_DTYPES = {"half": np.float16, "float": np.float32, "double": np.float64}
_MODELS = {
    "dsift": {"num_ang_bins": 8, "num_spatial_bins": 4, "spatial_bin_size": 4, "rootsift": True, "clipval": 0.2},
    "image": {"grayscale": False},
}


def _merge(base, over):
    out = copy.deepcopy(dict(base))
    for k, v in dict(over or {}).items():
        if isinstance(v, dict) and isinstance(out.get(k), dict):
            out[k] = _merge(out[k], v)
        else:
            out[k] = v
    return out


class FeatureExtractor:
    """pixsfm.features.FeatureExtractor(conf) for the weight-free models ("dsift", "image"), on the context's GPU.
    __call__(image, keypoints, keypoint_ids, as_dict, overwrite_sparse) -> one entry per pyramid level: dicts
    {"patches", "corners", "keypoint_ids", "metadata"} as tensor_to_fmap returns them (extractor.py:152-225), or FeatureMaps."""

    default_conf = {
        'device': 'auto',
        'dtype': 'half',
        'fast_image_load': False,
        'l2_normalize': True,
        'max_edge': 1600,
        'model': {
            "name": "s2dnet",
        },
        'patch_size': 16,
        'pyr_scales': [1.0],
        'resize': 'LANCZOS',
        'sparse': True,
        'use_cache': False,
        'overwrite_cache': False,
        'load_cache_on_init': False,
        'cache_format': 'chunked',
    }
    filters = ("BILINEAR", "BICUBIC", "LANCZOS")

    def __init__(self, conf=None, model=None, ctx=None):
        if model is not None:
            raise ValueError("custom models are not supported: the GPU path implements the weight-free models dsift / image")
        conf = _merge(self.default_conf, conf)
        name = conf["model"].get("name")
        if name in ("s2dnet", "vggnet"):
            raise ValueError("model %r needs learned weights and stays in PyTorch (the reference's FeatureExtractor); the GPU "
                             "extractor implements the weight-free models 'dsift' and 'image'" % name)
        if name not in _MODELS:
            raise ValueError("unknown feature model %r (supported: %s)" % (name, ", ".join(sorted(_MODELS))))
        extra = set(conf["model"]) - set(_MODELS[name]) - {"name"}
        if extra:
            raise ValueError("unknown parameters %s of model %r" % (sorted(extra), name))
        conf["model"] = _merge(dict(_MODELS[name], name=name), conf["model"])
        m = conf["model"]
        if name == "dsift":
            if m["num_ang_bins"] != 8 or m["num_spatial_bins"] != 4:
                raise ValueError("dsift: only num_ang_bins = 8 and num_spatial_bins = 4 (128 channels) are supported")
            s = m["spatial_bin_size"]
            if int(s) != s or s < 2 or s > 8 or int(s) % 2:
                raise ValueError("dsift: spatial_bin_size must be even, 2 .. 8 (got %r)" % (s,))
            if not float(m["clipval"]) > 0:
                raise ValueError("dsift: clipval must be positive")
            self.output_dims = [128]
        else:
            self.output_dims = [1 if m["grayscale"] else 3]
        if conf["use_cache"]:
            raise ValueError("use_cache: writing the H5 feature cache is not supported by the GPU extractor")
        if conf["dtype"] not in _DTYPES:
            raise ValueError("dtype must be one of %s" % sorted(_DTYPES))
        if conf["resize"] not in self.filters:
            raise ValueError("resize must be one of %s" % (self.filters,))
        ps = conf["patch_size"]
        if int(ps) != ps or not 1 <= ps <= 16:
            raise ValueError("patch_size must be 1 .. 16 (got %r)" % (ps,))
        if not len(conf["pyr_scales"]) or any(not float(p) > 0 for p in conf["pyr_scales"]):
            raise ValueError("pyr_scales must be positive")
        dev = str(conf["device"])
        if dev == "cpu":
            raise ValueError("device 'cpu': the extractor runs on the GPU only (there is no CPU path)")
        if dev not in ("auto", "cuda") and not re.fullmatch(r"cuda:\d+", dev):
            raise ValueError("device must be 'auto', 'cuda' or 'cuda:N' (got %r)" % dev)
        self.conf = conf
        self.device = dev
        self._ctx = ctx
        self.channels_per_level = []
        for _ in conf["pyr_scales"]:
            self.channels_per_level += self.output_dims

    @property
    def ctx(self):
        if self._ctx is None:
            from .keypoint_adjustment import default_context
            self._ctx = default_context()
        return self._ctx

    @property
    def dtype(self):
        return _DTYPES[self.conf["dtype"]]

    # -- host side: decoding, resize, grey conversion (PIL, as the reference) ----------------------------------------------
    def get_scaled_image_size(self, image, pyr_scale=1.0):
        w, h = image.size
        return [int(round(min(self.conf["max_edge"] / max(w, h), 1) * x * pyr_scale)) for x in [w, h]]

    def resize_image(self, image, pyr_scale):
        from PIL import Image
        w_new, h_new = self.get_scaled_image_size(image, pyr_scale)
        return image.resize((w_new, h_new), getattr(Image, self.conf["resize"]))

    def open_image(self, image):
        """A path (as the reference), a PIL image or a uint8 array -> PIL image (not yet decoded for a path)."""
        from PIL import Image
        if isinstance(image, Image.Image):
            return image
        if isinstance(image, (str, bytes)) or hasattr(image, "__fspath__"):
            return Image.open(image)
        a = np.asarray(image)
        if a.dtype != np.uint8:
            raise ValueError("image arrays must be uint8 (got %s)" % a.dtype)
        return Image.fromarray(a)

    def preprocess(self, image):
        """-> (list of model inputs per pyramid level, original (width, height)): the grey uint8 image for dsift (PIL
        convert("L"); the kernels apply / 255), a (C, h, w) float32 array / 255 for the image model."""
        img = self.open_image(image)
        size = img.size
        if self.conf["fast_image_load"] and hasattr(img, "draft"):
            img.draft("RGB", tuple(self.get_scaled_image_size(img, self.conf["pyr_scales"][0])))
        levels = []
        for pyr_scale in self.conf["pyr_scales"]:
            im = self.resize_image(img, pyr_scale)
            if self.conf["model"]["name"] == "dsift" or self.conf["model"]["grayscale"]:
                a = np.ascontiguousarray(np.asarray(im.convert("L")))
                levels.append(a if self.conf["model"]["name"] == "dsift" else (a.astype(np.float32) / np.float32(255))[None])
            else:
                a = np.asarray(im.convert("RGB")).astype(np.float32) / np.float32(255)
                levels.append(np.ascontiguousarray(a.transpose(2, 0, 1)))
        return levels, size

    # -- the device side -------------------------------------------------------------------------------------------------
    def extract_to_arena(self, arena, first, level_input, keypoints, image_size):
        """Patches [first, first + n) of `arena` from one level's model input (fused for dsift)."""
        if self.conf["model"]["name"] == "dsift":
            m = self.conf["model"]
            return arena.extract_dsift(first, level_input, keypoints, image_size, spatial_bin_size=m["spatial_bin_size"],
                                       rootsift=m["rootsift"], clipval=m["clipval"], l2_normalize=self.conf["l2_normalize"])
        return arena.extract(first, self._device_map(level_input), keypoints, image_size,
                             l2_normalize=self.conf["l2_normalize"])

    def _device_map(self, level_input):
        """(1, C, h, w) float32 torch tensor on the context's device: the model's output."""
        import torch
        from ..engine import dsift_dense
        if self.conf["model"]["name"] == "dsift":
            m = self.conf["model"]
            return dsift_dense(self.ctx, level_input, m["spatial_bin_size"], m["rootsift"], m["clipval"])
        t = torch.from_numpy(level_input[None]).to("cuda:%d" % self.ctx.device)
        torch.cuda.current_stream().synchronize()
        return t

    def __call__(self, image, keypoints=None, keypoint_ids=None, as_dict=True, overwrite_sparse=None):
        levels, size = self.preprocess(image)
        return [self.tensor_to_fmap(level, size, keypoints, keypoint_ids, as_dict=as_dict, overwrite_sparse=overwrite_sparse)
                for level in levels]

    def tensor_to_fmap(self, level_input, image_size, keypoints=None, keypoint_ids=None, as_dict=True, overwrite_sparse=None):
        """extractor.py:152-225 on one level's model input: the sparse / dense decision, then patches from the GPU."""
        from ..engine import PatchArena
        sparse = self.conf["sparse"] if overwrite_sparse is None else overwrite_sparse
        ps = int(self.conf["patch_size"])
        if keypoints is not None:
            keypoints = np.asarray(keypoints, dtype=np.float64).reshape(-1, 2)
            if keypoint_ids is None:
                keypoint_ids = list(range(keypoints.shape[0]))
            elif keypoints.shape[0] != len(keypoint_ids):
                raise ValueError("Number of provided keypoint_ids and keypoints do not match.")
        if sparse and keypoints is None:
            raise RuntimeError("Cannot run sparse feature extraction without any keypoints.")
        c = self.output_dims[0]
        h, w = level_input.shape[-2:]
        scale = np.array((w / image_size[0], h / image_size[1]))
        better_sparse = keypoints is not None and h * w * c > keypoints.shape[0] * ps * ps * c
        if sparse and better_sparse:
            n = keypoints.shape[0]
            arena = PatchArena(self.ctx, n, ps, ps, c, self.dtype)
            try:
                if n:
                    self.extract_to_arena(arena, 0, level_input, keypoints, image_size)
                patches, corners, _ = arena.download()
            finally:
                arena.close()
            data = {"patches": patches, "corners": corners.astype(np.int32), "keypoint_ids": keypoint_ids,
                    "metadata": {"scale": scale, "is_sparse": True, "patch_size": ps}}
        else:
            import torch
            fm = self._device_map(level_input)
            if self.conf["l2_normalize"]:
                fm = torch.nn.functional.normalize(fm, dim=1)
            fm = fm.to(getattr(torch, {"half": "float16", "float": "float32", "double": "float64"}[self.conf["dtype"]]))
            data = {"patches": np.ascontiguousarray(fm.permute(0, 2, 3, 1).cpu().numpy()),
                    "corners": np.array([[0.0, 0.0]]), "keypoint_ids": [kDenseId],
                    "metadata": {"scale": scale, "is_sparse": False, "patch_size": ps}}
        if as_dict:
            return data
        return FeatureMap(data["patches"], data["keypoint_ids"], data["corners"], data["metadata"])


def get_keypoints_and_ids(image_name, keypoints, req_keypoint_ids):
    """extract.py:22-33."""
    keypoints_i, keypoint_ids_i, num_req_kps = None, None, 0
    if keypoints is not None:
        keypoints_i = np.asarray(keypoints[image_name], dtype=np.float64).reshape(-1, 2)
        num_req_kps = keypoints_i.shape[0]
        if req_keypoint_ids is not None:
            keypoint_ids_i = np.asarray(req_keypoint_ids[image_name], dtype=np.int64).reshape(-1)
            num_req_kps = len(keypoint_ids_i)
            keypoints_i = keypoints_i[keypoint_ids_i, :]
    return keypoints_i, keypoint_ids_i, num_req_kps


def features_from_image_list(extractor, image_dir, image_list, keypoints=None, req_keypoint_ids=None, device=False):
    """pixsfm.extract.features_from_image_list (extract.py:58-150) without the H5 cache -> FeatureManager.
    device=False: host patches, as the reference.  device=True: every level is ONE PatchArena sized by the total number of
    keypoints, filled image by image by the fused kernel; the FeatureMaps hold ArenaPatch handles (the result
    load_features_from_cache(device=True) gives).  device=True is always sparse: one arena per level needs one patch shape."""
    conf = extractor.conf
    if keypoints is None and (conf["sparse"] or device):
        raise AttributeError("Keypoints required for sparse feature extract.")
    image_list = list(image_list)
    if not device:
        fm = FeatureManager([int(c) for c in extractor.channels_per_level])
        for name in image_list:
            kp, ids, n = get_keypoints_and_ids(name, keypoints, req_keypoint_ids)
            if keypoints is not None and n == 0:
                continue
            for level, data in enumerate(extractor(os.path.join(str(image_dir), name), kp, ids)):
                fm.fset(level).emplace(name, FeatureMap(data["patches"], data["keypoint_ids"], data["corners"], data["metadata"]))
        return fm
    from ..engine import PatchArena
    plan = OrderedDict()
    for name in image_list:
        kp, ids, n = get_keypoints_and_ids(name, keypoints, req_keypoint_ids)
        if n:
            plan[name] = (kp, list(range(n)) if ids is None else ids)
    total = sum(len(kp) for kp, _ in plan.values())
    ps = int(conf["patch_size"])
    fm = FeatureManager([int(c) for c in extractor.channels_per_level])
    arenas = []
    for level, c in enumerate(extractor.channels_per_level):
        arena = PatchArena(extractor.ctx, total, ps, ps, int(c), extractor.dtype) if total else None
        fm.fset(level).arena = arena
        arenas.append(arena)
    first = 0
    for name, (kp, ids) in plan.items():
        levels, size = extractor.preprocess(os.path.join(str(image_dir), name))
        for level, level_input in enumerate(levels):
            extractor.extract_to_arena(arenas[level], first, level_input, kp, size)
            fm.fset(level).emplace(name, fmap_from_arena(arenas[level], first, ids))
        first += len(kp)
    return fm


def extract_patchdata_from_graph(graph):
    """keypoint_adjustment/main.py:274-279: {image name: matched keypoint ids} of a match graph, in node order."""
    out = OrderedDict()
    for node in graph.nodes:
        out.setdefault(graph.image_id_to_name[node.image_id], []).append(int(node.feature_idx))
    return dict(out)


def features_from_graph(extractor, image_dir, graph, keypoints_dict=None, device=False):
    """extract.py:197-215: features of the matched keypoints of `graph`."""
    matched = extract_patchdata_from_graph(graph)
    return features_from_image_list(extractor, image_dir, list(matched.keys()), keypoints=keypoints_dict,
                                    req_keypoint_ids=matched, device=device)


def _project(camera, image, xyz):
    """Image coordinates of 3D points: pycolmap's cam.world_to_image(image.project(X)) where the objects have it, else the
    camera models of pixsfm_amd.synthetic.project."""
    if hasattr(camera, "world_to_image") and hasattr(image, "project"):
        return np.asarray(camera.world_to_image(image.project(list(xyz))), dtype=np.float64).reshape(-1, 2)
    from .. import synthetic
    params = np.asarray(camera.params, dtype=np.float64)
    return np.array([synthetic.project(camera.model_id, params, image.qvec, image.tvec, X) for X in xyz]).reshape(-1, 2)


def features_from_reconstruction(extractor, reconstruction, image_dir, device=False):
    """extract.py:153-194: features at the projections of the 3D points every registered image observes (keypoint ids =
    the observing point2D indices)."""
    image_list, keypoints_dict, keypoint_ids_dict = [], {}, {}
    for image_id, image in reconstruction.images.items():
        obs = [(i, p.point3D_id) for i, p in enumerate(image.points2D) if p.has_point3D()]
        if not obs:
            continue
        ids, p3d = zip(*obs)
        cam = reconstruction.cameras[image.camera_id]
        proj = _project(cam, image, [reconstruction.points3D[p].xyz for p in p3d])
        kp = np.zeros((len(image.points2D), 2), dtype=np.float64)
        kp[list(ids)] = proj
        image_list.append(image.name)
        keypoints_dict[image.name] = kp
        keypoint_ids_dict[image.name] = list(ids)
    return features_from_image_list(extractor, image_dir, image_list, keypoints=keypoints_dict,
                                    req_keypoint_ids=keypoint_ids_dict, device=device)
