"""pf3plat_amd — MI355X-native differentiable 3D-Gaussian rasterizer behind PF3plat's
`cuda_splatting` operator surface (C ABI in include/gsr.h)."""
from .types import DecoderOutput, DepthRenderingMode, Gaussians  # noqa: F401
from .rasterizer import (  # noqa: F401
    GaussianRasterizationSettings,
    GaussianRasterizer,
    RasterConfig,
    get_backend,
    pack_views,
    rasterize_views,
    views_from_cameras,
)
from .splatting import (  # noqa: F401
    render_cuda,
    render_cuda_orthographic,
    render_depth_cuda,
    render_views,
)
from .adapter import AdaptedGaussians, GaussianAdapter, GaussianAdapterCfg  # noqa: F401
from .decoder import DecoderSplattingCUDA, DecoderSplattingCUDACfg, get_decoder  # noqa: F401
from .geometry import depth_to_relative_disparity, get_fov, get_projection_matrix, homogenize_points  # noqa: F401

__version__ = "0.1.0"
from .ply_export import export_ply, gaussians_from_ply, read_ply  # noqa: F401,E402
from .sh_rotation import rotate_sh  # noqa: F401,E402
from . import losses  # noqa: F401,E402
from . import cost_volume  # noqa: F401,E402
from .cost_volume import depth_candidates, plane_sweep_cost_volume  # noqa: F401,E402
from . import pose  # noqa: F401,E402
from .pose import CoarsePoses, coarse_poses, pack_matches, pnp_ransac, synchronize_cameras  # noqa: F401,E402
from .pose import PoseErrors, RefinedPoses, pose_encoding, pose_errors, refine_poses  # noqa: F401,E402
from . import lift  # noqa: F401,E402
from .lift import LiftedDepth, lift_depth, plucker_rays  # noqa: F401,E402
from . import mono_attention  # noqa: F401,E402
from .mono_attention import mono_guided_attention  # noqa: F401,E402
from . import attention  # noqa: F401,E402
from .attention import CrossBlock, LearnableFourierPositionalEncoding, SelfBlock, apply_cached_rotary_emb  # noqa: F401,E402
from .attention import bidirectional_cross_attention, multi_head_attention, ragged_attention  # noqa: F401,E402
from . import matching  # noqa: F401,E402
from .matching import MatchAssignment, Matches, match_assignment, pack_matched  # noqa: F401,E402
from . import matcher  # noqa: F401,E402
from .matcher import LightGlue, TransformerLayer, pair_lists  # noqa: F401,E402
from . import keypoints  # noqa: F401,E402
from .keypoints import Keypoints, PackedKeypoints, SuperPoint, detect_keypoints, keypoints_from_scores  # noqa: F401,E402
from . import lpips  # noqa: F401,E402
from .lpips import LPIPS, load_lpips_state_dict, lpips_distance  # noqa: F401,E402
