"""jax_raft_amd: an MI355X (gfx950)-native RAFT optical-flow framework with the
API of alebeck/jax-raft (``RAFT``, ``raft_large``, ``raft_small``)."""
from .eval.metrics import flow_metrics, metrics_from, photometric_error
from .models.raft import RAFT, raft_large, raft_small
from .models.reference import (BidirectionalFlow, BidirectionalInterp, BidirectionalWarp, fb_consistency,
                               interpolate_frames, warp_frames)

__version__ = "0.1.0"
__all__ = ("RAFT", "raft_large", "raft_small", "BidirectionalFlow", "fb_consistency", "flow_metrics", "metrics_from",
           "BidirectionalWarp", "warp_frames", "photometric_error", "BidirectionalInterp", "interpolate_frames")
