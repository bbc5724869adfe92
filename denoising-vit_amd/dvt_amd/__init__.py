"""dvt_amd -- MI355X-native DVT stage-1 denoising (hash-grid field + fused fit + ViT
extractor) behind the reference's `dvt.models` API.  See DESIGN.md."""
from . import _lib  # noqa: F401
from . import vit  # noqa: F401  (registers the ViT entry points before the first library load)
from . import s2  # noqa: F401  (stage-2 entry points)
from . import denoiser_bf16  # noqa: F401  (the denoiser's bf16 inference entry points)
from . import s3  # noqa: F401  (stage-3 entry points)
from . import seg  # noqa: F401  (segmentation-evaluation entry points)
from . import depth  # noqa: F401  (depth-evaluation entry points)
from . import vis  # noqa: F401  (visualisation entry points)
from . import video  # noqa: F401  (video-demo entry points)
from .fit import FitEngine, FitSettings  # noqa: F401
from . import models  # noqa: F401

__all__ = ["FitEngine", "FitSettings", "models", "vit"]
