"""The `_pixsfm`-shaped adapter (pixsfm_amd/_pixsfm): its surface is checked against the names the reference's modules import.
`reference_pixsfm` registers the adapter as `pixsfm._pixsfm` (with minimal stand-ins for omegaconf / pyceres / pycolmap, absent
in this image) so that the reference's own, unmodified L4 Python can be imported on top of it from a reference checkout; the
golden generator tests/golden/make_golden_defaults.py uses it to read the reference's default_conf dictionaries."""
import importlib
import logging
import os
import sys
import types

import numpy as np
import pytest

REF = "/root/reference/pixsfm"


class _Cfg(dict):
    """OmegaConf stand-in: nested dict with attribute access."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    @staticmethod
    def wrap(d):
        if isinstance(d, dict):
            return _Cfg({k: _Cfg.wrap(v) for k, v in d.items()})
        if isinstance(d, (list, tuple)):
            return [_Cfg.wrap(v) for v in d]
        return d

    @staticmethod
    def unwrap(d):
        if isinstance(d, dict):
            return {k: _Cfg.unwrap(v) for k, v in d.items()}
        if isinstance(d, list):
            return [_Cfg.unwrap(v) for v in d]
        return d


def _merge(a, b):
    out = dict(a)
    for k, v in (b or {}).items():
        out[k] = _merge(out[k], v) if isinstance(v, dict) and isinstance(out.get(k), dict) else v
    return out


@pytest.fixture()
def reference_pixsfm():
    if not os.path.isdir(REF):
        pytest.skip("reference tree absent")
    saved = dict(sys.modules)
    import pixsfm_amd._pixsfm as shim
    om = types.ModuleType("omegaconf")

    class OmegaConf:
        @staticmethod
        def create(d=None):
            return _Cfg.wrap(d or {})

        @staticmethod
        def merge(*confs):
            acc = {}
            for c in confs:
                acc = _merge(acc, _Cfg.unwrap(c))
            return _Cfg.wrap(acc)

        @staticmethod
        def to_container(cfg, resolve=False):
            return _Cfg.unwrap(cfg)

        @staticmethod
        def resolve(cfg):
            pass
    om.OmegaConf, om.DictConfig = OmegaConf, _Cfg
    om_sub = types.ModuleType("omegaconf.omegaconf")
    om_sub.OmegaConf, om_sub.DictConfig = OmegaConf, _Cfg
    om.omegaconf = om_sub
    sys.modules["omegaconf.omegaconf"] = om_sub
    pyceres = types.ModuleType("pyceres")
    pyceres.ListIterationCallback = list
    pyceres.IterationCallback = object
    from pixsfm_amd.api import reconstruction as rec_mod
    pycolmap = types.ModuleType("pycolmap")
    pycolmap.Reconstruction = rec_mod.Reconstruction
    pkg = types.ModuleType("pixsfm")
    pkg.__path__ = [REF]
    pkg.logger = logging.getLogger("pixsfm-test")
    sys.modules.update({"omegaconf": om, "pyceres": pyceres, "pycolmap": pycolmap, "pixsfm": pkg})
    shim.install_as("pixsfm._pixsfm")
    # pixsfm/features/__init__.py also pulls in the CNN extractors (torch models, h5py writers): out of scope here,
    # so `pixsfm.features` is the native half of that package only
    feats = types.ModuleType("pixsfm.features")
    feats.__dict__.update({k: v for k, v in vars(shim._features).items() if not k.startswith("__")})
    sys.modules["pixsfm.features"] = feats
    pkg.features = feats
    yield importlib.import_module
    for k in list(sys.modules):                 # only what this fixture registered (never torch & co.)
        if k == "pixsfm" or k.startswith("pixsfm.") or k in ("omegaconf", "omegaconf.omegaconf", "pyceres", "pycolmap"):
            if k in saved:
                sys.modules[k] = saved[k]
            else:
                del sys.modules[k]


def test_adapter_exports_what_the_reference_modules_import():
    import pixsfm_amd._pixsfm as shim
    want = {
        "_base": ["Graph", "FeatureNode", "Match", "InterpolationConfig", "InterpolatorType", "Map_NameKeypoints",
                  "compute_track_labels", "compute_score_labels", "compute_root_labels", "count_track_edges", "count_edges_AB"],
        "_features": ["FeaturePatch", "FeatureMap", "FeatureSet", "FeatureView", "FeatureManager", "Reference",
                      "PatchInterpolator", "kDenseId", "FeatureSet_f16", "FeatureManager_f32"],
        "_keypoint_adjustment": ["FeatureMetricKeypointOptimizer", "TopologicalReferenceKeypointOptimizer",
                                 "KeypointAdjustmentSetup", "KeypointOptimizerOptions"],
        "_bundle_adjustment": ["FeatureReferenceBundleOptimizer", "ReferenceExtractor", "BundleAdjustmentSetup",
                               "CostMapExtractor", "CostMapBundleOptimizer", "BundleOptimizerOptions",
                               "PatchWarpBundleOptimizer", "GeometricBundleOptimizer"],
        "_localization": ["QueryKeypointOptimizer", "QueryBundleOptimizer", "find_nearest_references"],
        "_util": ["free_memory", "total_memory", "used_memory"],
    }
    for sub, names in want.items():
        for n in names:
            assert hasattr(getattr(shim, sub), n), (sub, n)
    with pytest.raises(NotImplementedError):
        shim._bundle_adjustment.PatchWarpBundleOptimizer({}, None, {})
    assert shim._util.total_memory() >= shim._util.free_memory() > 0
