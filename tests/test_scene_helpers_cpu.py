"""The helpers the whole-scene test paths of mvpnet_amd/scene.py share, on CPU tensors: the eval scope, the frame store, the bucket
placement and the resize rule."""
import pytest
import torch


def test_the_eval_scope_restores_the_mode_and_the_gradients_when_the_body_raises():
    from mvpnet_amd.nn import eval_mode
    model = torch.nn.Linear(2, 2)
    for training in (True, False):
        model.train(training)
        assert torch.is_grad_enabled()
        with pytest.raises(ZeroDivisionError):
            with eval_mode(model):
                assert not model.training and not torch.is_grad_enabled()
                1 / 0
        assert model.training is training and torch.is_grad_enabled()
        with eval_mode(model):
            assert not model.training and not model(torch.ones(1, 2)).requires_grad
        assert model.training is training and torch.is_grad_enabled()


def test_infer_scene_restores_the_mode_when_a_forward_raises():
    from mvpnet_amd.scene import infer_scene

    class Raises(torch.nn.Module):
        num_classes = 2

        def forward(self, data):
            raise ValueError('no forward today')

    for training in (True, False):
        model = Raises().train(training)
        with pytest.raises(ValueError):
            infer_scene(model, [{'points': torch.zeros(1, 3, 8)}], [torch.arange(8)], 8)
        assert model.training is training


C, H, W, F, FRAMES = 4, 3, 5, 9, [1, 4, 5, 8]


class Counting2D(torch.nn.Module):
    """Elementwise, so the batch size cannot change a bit; element (0,0,0) of image f is f: the frames it sees are listed in `seen`."""

    def __init__(self):
        super().__init__()
        self.seen, self.batches = [], []

    def forward(self, data):
        x = data['image']
        self.seen += [int(v) for v in x[:, 0, 0, 0]]
        self.batches.append(x.size(0))
        return {'out': torch.stack([x[:, 0] * (c + 1) + x[:, 1] * 0.5 - x[:, 2] for c in range(C)], 1)}


def _images():
    images = torch.randn(F, 3, H, W, generator=torch.Generator().manual_seed(4))
    images[:, 0, 0, 0] = torch.arange(F, dtype=torch.float32)
    return images


def _store(net, channels=None):
    from mvpnet_amd import scene as S
    run = S._frames_through(net, 'out', _images(), None, False)
    return S._frame_store(FRAMES, F, H, W, 3, run, 'test', torch.device('cpu'), channels)


@pytest.mark.parametrize('channels', [None, C])
def test_the_frame_store_holds_every_distinct_frame_once_in_channels_last_memory(channels):
    net = Counting2D()
    store, slot_of = _store(net, channels)
    assert net.seen == FRAMES and net.batches == [3, 1], 'every frame once, the last forward partial'
    assert tuple(store.shape) == (len(FRAMES), H, W, C) and store.dtype == torch.float32 and store.is_contiguous()
    logit = store.permute(0, 3, 1, 2)
    assert tuple(logit.shape) == (len(FRAMES), C, H, W) and logit.stride(1) == 1
    assert slot_of.dtype == torch.int32 and tuple(slot_of.shape) == (F,)
    assert slot_of.tolist() == [FRAMES.index(f) if f in FRAMES else -1 for f in range(F)]
    images = _images()
    for f in FRAMES:
        want = Counting2D()({'image': images[f:f + 1]})['out'][0]
        assert torch.equal(store[slot_of[f]], want.permute(1, 2, 0))


def test_the_frame_store_refuses_another_output():
    class Half(Counting2D):
        def forward(self, data):
            return {'out': super().forward(data)['out'].half()}

    class Small(Counting2D):
        def forward(self, data):
            return {'out': super().forward(data)['out'][:, :, ::2, ::2].contiguous()}

    for net, channels in ((Half(), None), (Half(), C), (Small(), None), (Small(), C), (Counting2D(), C + 1)):
        with pytest.raises(RuntimeError, match='test: net_2d must return a float32'):
            _store(net, channels)


def test_the_bucket_placement_is_the_one_the_2d_path_computed_by_hand():
    from mvpnet_amd import scene as S
    lengths = [1, 5, 5, 64, 65, 700, 33000]
    # the loop _scene_2d_inputs held before it called _bucketed_rows
    batches, _ = S.plan_buckets(lengths, min_nb_pts=1)
    out_base, out_len, knn_base, at, rows = [0] * len(lengths), [0] * len(lengths), [0] * len(lengths), 0, 0
    for N, members in batches:
        for c in members:
            out_base[c], out_len[c], knn_base[c], at, rows = at, N, rows, at + 3 * N, rows + N
    got_batches, order, slot_base, got_len = S._bucket_slots(lengths, 'test', 1, 32, 32 * 8192, 32768)
    assert got_batches == batches and got_len == out_len
    assert slot_base == [b // 3 for b in out_base] and [3 * s for s in slot_base] == out_base and slot_base == knn_base
    assert [c for _, members in got_batches for c in members] == order and sorted(order) == list(range(len(lengths)))
    assert sum(N * len(members) for N, members in got_batches) == rows
    assert len(batches) > 2 and all(n <= N for n, N in zip(lengths, out_len)) and out_len[-1] == 33000
    with pytest.raises(RuntimeError):
        S._bucket_slots([3, 0], 'test', 1, 32, 32 * 8192, 32768)


def test_the_resize_target():
    from mvpnet_amd.scene import _resize_target
    assert _resize_target(None, 160, 120) is None and _resize_target((), 160, 120) is None and _resize_target([], 160, 120) is None
    assert _resize_target((160, 120), 160, 120) is None and _resize_target([160.0, 120.0], 160, 120) is None
    assert _resize_target((120, 160), 160, 120) == (120, 160)
    got = _resize_target([80.0, 60.0], 160, 120)
    assert got == (80, 60) and all(type(v) is int for v in got)
