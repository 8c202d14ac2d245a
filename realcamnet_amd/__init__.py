"""realcamnet_amd -- MI355X (gfx950) native RAW->sRGB learned-ISP inference path.

Host-side mirror of the reference interface (kepengxu/RealCamNet models/networks.py, models/LiteISP.py)
over the C ABI in include/realcam_hip.h (librealcam_hip.so, hand-written HIP).  No CPU fallback.
"""
from . import networks  # noqa: F401
from . import LiteISP  # noqa: F401
from . import groupmix  # noqa: F401
from . import tcm  # noqa: F401
from . import raw2bit  # noqa: F401
from . import graphs  # noqa: F401
from .graphs import GraphedCall  # noqa: F401
from .LiteISP import (ISPUNet_GFM, ISPUNet_GFM_crop, ISPUNet_GFM_LFM, ISPUNet_GFM_LSC, ISPUNet_GFM_LSC1, ISPUNet_GFM_LSC_noskip, ISPUNet_LSC, LiteISPNet, LiteISPNet_GFM, LiteISPNet_GFM_LSC,  # noqa: F401
                      LiteISPNet_GFM_LSC_GMA, LiteISPNet_GFMresize, LiteISPNet_LSC, ResUNet)
from .groupmix import GMA_Block  # noqa: F401
from .raw_format import RawFormat  # noqa: F401
from .raw_stats import RawFrameStats, RawStats  # noqa: F401
from .raw_noise import RawNoise, RawNoiseStats  # noqa: F401
from .aberration import Aberration  # noqa: F401
from .out_format import OutFormat, YuvFrames  # noqa: F401
from .jpeg import Jpeg, JpegFrames  # noqa: F401
from .dng import Dng, DngFrames  # noqa: F401
from .look import Lut3D  # noqa: F401
from .warp import Warp  # noqa: F401
from .stats import FrameStats, Stats  # noqa: F401
from .motion import Motion, MotionField, MotionState, Stabilizer  # noqa: F401
from .resize import Output, Resize  # noqa: F401
from .sharpen import Sharpen  # noqa: F401
from .tone import ToneMap  # noqa: F401
from .defects import DefectMap, Defects  # noqa: F401
from .calibration import Calibration, GainMap, Pwl  # noqa: F401
from .exposures import Exposures  # noqa: F401
from .temporal import Temporal, TemporalMotion, TemporalState  # noqa: F401
from .quad import QuadBayer  # noqa: F401

__all__ = ["networks", "LiteISP", "groupmix", "tcm", "raw2bit", "LiteISPNet", "LiteISPNet_GFM_LSC", "LiteISPNet_GFM_LSC_GMA", "LiteISPNet_LSC",
           "LiteISPNet_GFM", "LiteISPNet_GFMresize", "ISPUNet_GFM_LSC", "ISPUNet_GFM", "ISPUNet_GFM_LFM", "ISPUNet_LSC", "ResUNet", "ISPUNet_GFM_crop", "ISPUNet_GFM_LSC1",
           "ISPUNet_GFM_LSC_noskip", "GMA_Block", "graphs", "GraphedCall", "RawFormat", "OutFormat", "YuvFrames", "Jpeg", "JpegFrames", "Dng", "DngFrames", "Resize", "Output", "Lut3D", "Warp", "Stats", "FrameStats", "Motion", "MotionField", "MotionState", "Stabilizer", "DefectMap", "Defects", "Calibration", "GainMap", "Pwl", "Exposures", "Temporal", "TemporalMotion", "TemporalState", "Sharpen", "ToneMap", "QuadBayer", "RawStats", "RawFrameStats", "RawNoise", "RawNoiseStats", "Aberration"]
