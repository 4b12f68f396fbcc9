"""pcl_feature_extraction_amd -- MI355X-native (gfx950) hot path of srv/pcl_feature_extraction.

NARF keypoints on the planar range image + normals + FPFH-33 / SHOT-352 / SHOT-1344 / PFH-125 / spin-image /
intensity-gradient / RIFT / intensity-spin / 3D-shape-context / unique-shape-context / moment-invariant / principal-curvature / NARF-36 / CVFH descriptors, BOARD local reference frames and boundary points over radius neighbourhoods, descriptor matching, RANSAC rejection and ICP
alignment, as hand-written HIP kernels behind the C-ABI in include/pfx.h (libpfx.so).
See DESIGN.md.
"""
from ._native import BOUNDARY_NO_NEIGHBORS, PfxError, lib  # noqa: F401
from .api import (Batch, Context, Cvfh, IcpResult, NarfDescriptors, board_params, camera, cvfh_params,  # noqa: F401
                  icp_params, narf_desc_params, narf_params, rgb_to_intensity, spin_params, uniform01_stream)

__all__ = ["BOUNDARY_NO_NEIGHBORS", "Batch", "Context", "Cvfh", "IcpResult", "NarfDescriptors", "PfxError", "board_params",
           "camera", "cvfh_params", "icp_params", "narf_desc_params", "narf_params", "rgb_to_intensity", "spin_params", "uniform01_stream", "lib"]
