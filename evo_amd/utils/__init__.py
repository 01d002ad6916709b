from .prepost import (  # noqa: F401
    MultiDimOverlappingPatches,
    OverlappingPatches,
    mean_merger,
    median_merger,
    psnr,
)
