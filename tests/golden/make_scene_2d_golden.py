"""Writes tests/golden/scene_2d.npz: the whole-scene test of the 2D baseline as the reference runs it (mvpnet/test_2d_chunks.py:119-157),
chunk by chunk on the CPU over a small synthetic scene.

    python -m tests.golden.make_scene_2d_golden

What is the reference's: scene2chunks_legacy (mvpnet/utils/chunk_util.py, imported), select_frames (scannet_2d3d.py:20-30; that module
imports open3d, so its 9 lines are re-typed as in make_golden.gen_chunker), MVPNet2D (mvpnet/models/mvpnet_2d.py, imported, group_points
stubbed by its own test oracle: make_golden.install_reference) and the accumulation of test_2d_chunks.py:132-157, re-typed.  The overlap
comes from tests/scene_prep_oracle.rgbd_overlap, the pixel k-NN indices from oracle.c_oracle.unproject / pixel_knn with the chunk boxes
(-/+ 0.1 m), the 2D network is the stand-in of tests/lift_vote_oracle (20 logits from the three image channels, every operation rounded
once).  Scene and parameters: lift_vote_oracle.FIXTURE -- 12 frames and a threshold of 150 points: with fewer frames or smaller chunks some
chunk's views hold no valid pixel inside its box, and the reference's loader cannot build such a chunk (its ball tree has nothing to fit).

The script insists that the scene has a point in no chunk and a chunk whose base points no frame sees, that every chunk finds k valid
pixels (the reference cannot run otherwise), that the float32 oracle and the reference lie within the rounding bound of the script's own
float64 evaluation, and that fewer than 0.5 % of the voted points have a float64 top-two gap inside twice that bound."""
import os

import numpy as np
import torch

from tests.golden import make_golden as MG
from tests import lift_vote_oracle as LO
from tests import scene_prep_oracle as SO
from oracle import c_oracle as O


def select_frames(rgbd_overlap, num_rgbd_frames):  # scannet_2d3d.py:20-30
    selected_frames = []
    rgbd_overlap = rgbd_overlap.copy()
    for i in range(num_rgbd_frames):
        frame_idx = rgbd_overlap.sum(0).argmax()
        selected_frames.append(frame_idx)
        rgbd_overlap[rgbd_overlap[:, frame_idx]] = False
    return selected_frames


class StandIn(torch.nn.Module):
    def forward(self, data):
        x, w = data['image'], torch.from_numpy(LO.standin_weights())
        return {'seg_logit': torch.stack([(x[:, 0] * w[0, c] + x[:, 1] * w[1, c]) + x[:, 2] * w[2, c] for c in range(w.size(1))], 1)}


def chunk_knn(sc, picks, box, pts, k):
    """One chunk's k-NN rows: its own views and box, as the loader does (scannet_2d3d.py:254-313)."""
    depth = O.depth_mm_to_m(sc['depth_mm'][picks])[None]
    kinv = np.repeat(sc['kinv'][None], len(picks), 0)[None]
    xyz, mask = O.unproject(depth, kinv, sc['pose'][picks][None], box[None])
    return O.pixel_knn(xyz, mask, pts[None], k)[0], int(mask.sum())


def main():
    MG.install_reference()
    from mvpnet.utils.chunk_util import scene2chunks_legacy
    from mvpnet.models.mvpnet_2d import MVPNet2D
    P = LO.FIXTURE
    sc = LO.fixture_scene()
    points, n_pts, k, nv, hw = sc['points'], P['n_pts'], P['k'], P['num_rgbd_frames'], P['h'] * P['w']
    chunk_inds, boxes = scene2chunks_legacy(points, P['chunk_size'], P['chunk_stride'], thresh=P['chunk_thresh'], margin=P['chunk_margin'],
                                            return_bbox=True)
    base = sc['base_point_ind']
    overlaps = SO.rgbd_overlap(sc['depth_mm'], sc['kinv'], sc['pose'], points[base], P['radius'])
    masks = SO.chunk_masks_of(chunk_inds, base, n_pts)
    picked = np.array([select_frames(overlaps[m], nv) for m in masks], np.int64)
    unseen = [c for c, m in enumerate(masks) if not overlaps[m][:, picked[c]].any()]
    print('%d chunks, lengths %s, chunks no frame sees: %s' % (len(chunk_inds), [len(i) for i in chunk_inds], unseen))
    assert unseen, 'the scene needs a chunk whose base points no frame sees'

    model = MVPNet2D(StandIn()).eval()
    num_classes = LO.STANDIN_CLASSES
    pred_logit_whole_scene = np.zeros([n_pts, num_classes], dtype=np.float32)   # test_2d_chunks.py:132-133
    num_pred_per_point = np.zeros(n_pts, dtype=np.uint8)
    knn_rows = []
    with torch.no_grad():
        for c, chunk_ind in enumerate(chunk_inds):
            box = (np.asarray(boxes[c], np.float64)[[0, 1, 3, 4]] + np.array([-0.1, -0.1, 0.1, 0.1])).astype(np.float32)
            knn, valid = chunk_knn(sc, picked[c], box, points[chunk_ind], k)
            assert valid >= k and knn.min() >= 0, 'chunk %d finds %d valid pixels' % (c, valid)
            knn_rows.append(knn)
            data_batch = {'images': torch.from_numpy(sc['images'][picked[c]])[None], 'knn_indices': torch.from_numpy(knn)[None]}
            preds = model(data_batch)
            seg_logit = preds['seg_logit'].squeeze(0).cpu().numpy().T
            seg_logit = seg_logit[:len(chunk_ind)]
            pred_logit_whole_scene[chunk_ind] += seg_logit                   # :146-147
            num_pred_per_point[chunk_ind] += 1
    pred_logit_whole_scene = pred_logit_whole_scene / np.maximum(num_pred_per_point[:, np.newaxis], 1)   # :150-157
    pred_label_whole_scene = np.argmax(pred_logit_whole_scene, axis=1)
    pred_label_whole_scene[num_pred_per_point == 0] = num_classes
    assert pred_logit_whole_scene.dtype == np.float32
    assert (num_pred_per_point == 0).any(), 'the scene needs a point in no chunk'
    assert num_pred_per_point.max() > 1, '... and a point in several'

    # the script's own float64 evaluation, the bound and the 0.5 % cap -- for the reference's result and for the float32 oracle's
    frames = np.unique(picked)
    view_frame = np.searchsorted(frames, picked).astype(np.int32)
    store = LO.standin_logits(sc['images'][frames]).reshape(len(frames), num_classes, hw).transpose(0, 2, 1)
    lengths = np.array([len(i) for i in chunk_inds], np.int64)
    knn_base = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    knn_all = np.concatenate(knn_rows)
    total64, scale, count = LO.lift_vote_f64(store, view_frame, knn_all, knn_base, chunk_inds, n_pts)
    assert np.array_equal(count, num_pred_per_point.astype(np.int32))
    worst, excluded = LO.check_against_f64(pred_logit_whole_scene, pred_label_whole_scene, count, total64, scale, k)
    print('reference vs float64: worst error / bound %.3f, %.4f %% of the voted points excluded from the label comparison' % (worst, 100 * excluded))
    mean32, label32 = LO.finish(*LO.lift_vote_f32(np.ascontiguousarray(store), view_frame, knn_all, knn_base, chunk_inds, n_pts))
    worst, excluded = LO.check_against_f64(mean32, label32, count, total64, scale, k)
    print('float32 oracle vs float64: worst error / bound %.3f; bit-equal to the reference on %.2f %% of the elements' % (
        worst, 100 * float((mean32 == pred_logit_whole_scene).mean())))
    print('%d distinct picked frames of %d chunk views, %d points without a chunk' % (len(frames), picked.size, int((count == 0).sum())))

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'scene_2d.npz')
    np.savez_compressed(path, base_point_ind=base.astype(np.int32), overlaps=np.packbits(overlaps, axis=1), picked=picked.astype(np.int16),
                        lengths=lengths.astype(np.int32), chunk_index=np.concatenate(chunk_inds).astype(np.int32), knn=knn_all.astype(np.int16),
                        mean=pred_logit_whole_scene, label=pred_label_whole_scene.astype(np.int8), count=num_pred_per_point)
    print('wrote', path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1000000


if __name__ == '__main__':
    main()
