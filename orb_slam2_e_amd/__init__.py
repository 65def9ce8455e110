"""MI355X-native front-end hot path of ORB_SLAM2_E (ORB extract, Hamming match, FEM).

The compute path is hand-written HIP for gfx950 behind the C-ABI declared in
include/*.h (liborbslam_hip.so); this package is the thin host-side mirror of the
reference's ORBextractor / ORBmatcher / FEA2 interfaces used by tests and bench.
"""
from ._lib import OrbxError, build, lib  # noqa: F401
from .extractor import KP_DTYPE, ComputeStereoMatches, ORBextractor, extract_pair, stereo_download_batch, stereo_match_batch  # noqa: F401
from .matcher import Distortion, Frame, FuseTarget, MapSnapshot, ORBmatcher, Points, TriangKeyFrame, View, image_bounds, undistort_points  # noqa: F401
from .pose import PoseCamera, PoseStats, pose_optimization, pose_optimization_batch, pose_optimization_batch_device  # noqa: F401
from .pose import pose_optimization_nr, pose_optimization_nr_batch  # noqa: F401
from .sim3 import (RefineSim3Attempt, Sim3OptProblem, Sim3Problem, Sim3Solver, first_accepted, optimize_sim3,  # noqa: F401
                   refine_sim3_candidates, sim3_hypotheses)
from .initializer import Initializer, check_rt, find_models, last_init_waits, reconstruct_f  # noqa: F401
from .keyframe_database import KeyFrameDatabase  # noqa: F401
from .pnp import PnPsolver, PnpProblem, pnp_hypotheses  # noqa: F401
from .bundle import (BaGraph, BaOptions, BaResult, BaStats, bundle_adjustment, global_bundle_adjustment,  # noqa: F401
                     global_bundle_adjustment_env, llt_env_plan, llt_env_solve_device, llt_solve_device, local_bundle_adjustment)
from .essential_graph import EgGraph, EgOptions, EgResult, EgStats  # noqa: F401
from .essential_graph import optimize as optimize_essential_graph  # noqa: F401
from .essential_graph import optimize_env as optimize_essential_graph_env  # noqa: F401
