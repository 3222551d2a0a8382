"""gitcap: MI355X-native GIT-style video-caption inference behind the call surface of
farazali7/real-time-video-captioning (see DESIGN.md / INTEGRATION.md)."""
from .config import GitCapConfig, git_base, git_large, git_tiny          # noqa: F401
from .weights import synthetic_weights, canonical_shapes                  # noqa: F401


def __getattr__(name):
    # GitCaptioner pulls in torch + the HIP library; keep `import gitcap` light for host-only tools
    if name == "GitCaptioner":
        from .model import GitCaptioner
        return GitCaptioner
    if name == "draft_and_verify":
        from .model import draft_and_verify
        return draft_and_verify
    if name == "caption_confidence":
        from .confidence import caption_confidence
        return caption_confidence
    if name == "frame_attribution":
        from .confidence import frame_attribution
        return frame_attribution
    if name == "soft_labels":
        from .scoring import soft_labels
        return soft_labels
    if name == "distill_report":
        from .distill import distill_report
        return distill_report
    if name in ("sample_frames", "caption_videos", "FrameSelection"):
        from . import sampling
        return getattr(sampling, name)
    if name in ("TeacherStreamPool", "StudentStreamPool"):
        from . import streampool
        return getattr(streampool, name)
    raise AttributeError(name)
