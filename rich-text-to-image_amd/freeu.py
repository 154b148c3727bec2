"""FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net"; diffusers >= 0.21 `pipe.enable_freeu(s1, s2, b1, b2)`): in the first two up
blocks of the UNet half of the backbone channels are amplified by b1 / b2 and the four lowest spatial frequency bins of the skip
features are scaled by s1 / s2 (diffusers' fourier_filter with its fixed threshold = 1).  No weights, no training.  The operator runs
inside the engine (csrc/freeu.hip, include/rtdiff.h: rt_set_freeu); this module holds the host side both pipelines share: the checked
setting, the pipeline attribute `freeu` and its way onto whichever engine a sampling call builds or reuses."""
import math

OFF = (1.0, 1.0, 1.0, 1.0)


def check_freeu(values, who="freeu"):
    """(s1, s2, b1, b2) -> a tuple of four finite floats > 0 (diffusers' argument order); anything else raises ValueError."""
    try:
        v = tuple(float(x) for x in values)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: expected four numbers s1 s2 b1 b2, got {values!r}")
    if len(v) != 4:
        raise ValueError(f"{who}: expected four numbers s1 s2 b1 b2, got {len(v)}")
    if not all(math.isfinite(x) and x > 0.0 for x in v):
        raise ValueError(f"{who}: s1, s2, b1, b2 must be finite and > 0, got {v}")
    return v


class FreeUMixin:
    """`enable_freeu(s1, s2, b1, b2)` / `disable_freeu()` of a pipeline: the setting is the attribute `freeu` (None = off), read by every
    sampling call - the plain pass, the token-map pass and the rich pass alike - when it has its engine (apply_freeu)."""
    freeu = None

    def enable_freeu(self, s1, s2, b1, b2):
        self.freeu = check_freeu((s1, s2, b1, b2), f"{type(self).__name__}.enable_freeu")

    def disable_freeu(self):
        self.freeu = None

    def apply_freeu(self, eng):
        """The pipeline's setting - else the one its UNet object carries (HipUNet2DConditionModel.enable_freeu), else off - onto `eng`."""
        eng.set_freeu(*(self.freeu or getattr(getattr(self, "unet", None), "freeu", None) or OFF))
