"""GPU: pxr_ba_eval refuses an fp16 patch larger than 4 GiB.  The fp16 path of the residual kernel addresses the 4 x 4 stencil with
32-bit byte offsets inside the patch; beyond 4 GiB they would wrap to other texels of the same patch (wrong values, no fault), so
the call must fail before any launch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_fp16_patch_over_4_gib_is_refused(ctx):
    from pixsfm_amd import synthetic
    from pixsfm_amd._lib import PixsfmHipError
    from pixsfm_amd.engine import BAProblem, PatchArena, interp_cfg
    prob = synthetic.make_ba_problem(n_cams=2, n_points=1, obs_per_point=1, channels=128, patch_size=16)
    H, W = 4096, 4097                     # 4096 x 4097 x 128 x 2 B = 4 GiB + 1 MiB, allocated: nothing outside it is ever addressed
    arena = PatchArena(ctx, 1, H, W, 128, np.float16)
    try:
        ba = BAProblem(ctx, arena, prob)
        with pytest.raises(PixsfmHipError, match="exceeds 4 GiB"):
            ba.eval(interp_cfg(), with_jacobian=True)
    finally:
        arena.close()
