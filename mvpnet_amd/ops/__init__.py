"""Host-side mirror of the reference's `mvpnet.ops` package (same function names, argument
meaning, defaults and autograd behaviour; reference: mvpnet/ops/*.py), running on
libmvp_hip.so through mvpnet_amd.ext.  GPU only -- no CPU fallback."""
from .fps import farthest_point_sample
from .ball_query import ball_query, ball_query_distance
from .group_points import group_points
from .knn_distance import knn_distance
from .interpolate import feature_interpolate
from .lifting import unproject, pixel_knn, lift_gather, lift_gather_backward, lift, lift_store, rotate_rows
from .overlap import rgbd_overlap, select_frames_batched, pack_bits, unpack_bits
from .vote import vote_nearest, lift_vote, vote_finish
from .sample import sample_chunks
from .scene_sample import sample_scenes, gather_cloud
from .chunker import scene_chunks, pack_chunks, pack_cloud
from .ensemble import ensemble_softmax, label_confusion
from .frames import prepare_frames
from .resize import resize_frames, prepare_labels
from .frame_eval import frame_confusion, label_histogram
from .fuse_cloud import CloudFuser, fuse_cloud

__all__ = ['farthest_point_sample', 'ball_query', 'ball_query_distance', 'group_points', 'knn_distance',
           'feature_interpolate', 'unproject', 'pixel_knn', 'lift_gather', 'lift_gather_backward', 'lift', 'lift_store', 'rotate_rows', 'rgbd_overlap', 'select_frames_batched',
           'pack_bits', 'unpack_bits', 'vote_nearest', 'lift_vote', 'vote_finish', 'sample_chunks', 'sample_scenes', 'gather_cloud', 'scene_chunks', 'pack_chunks',
           'pack_cloud', 'ensemble_softmax', 'label_confusion',
           'prepare_frames', 'resize_frames', 'prepare_labels', 'frame_confusion', 'label_histogram', 'CloudFuser', 'fuse_cloud']


def as_point_major(x, transpose):
    """(B,3,N) -> contiguous (B,N,3) when `transpose` (the reference wrappers' convention,
    e.g. mvpnet/ops/fps.py:28-30); otherwise just make it contiguous."""
    return (x.transpose(1, 2) if transpose else x).contiguous()
