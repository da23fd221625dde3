"""mvp_lift_vote_f32 on the MI355X against the float32 oracle (tests/lift_vote_oracle.py), bit for bit, at the smallest shapes where it
can go wrong: ragged chunks whose k-NN rows are not back to back (the rows between them hold ids far out of range), points in no, one
and every chunk, two chunks sharing a frame in different view slots, missing neighbours, class counts that take the 16-byte and the
dword path and leave the last workgroup partial, channels-last / NCHW / 4-byte-aligned stores; run twice; replayed from a graph."""
import numpy as np
import pytest
import torch

from tests import lift_vote_oracle as LO

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
U, H, W, NV, N_PTS = 5, 6, 8, 3, 300
LENGTHS = [70, 1, 257, 64]
GAPS = [3, 0, 10, 58, 5]   # rows of knn before chunk 0, between the chunks, and behind the last
VIEW_FRAME = np.array([[0, 1, 2], [2, 0, 4], [3, 3, 1], [4, 2, 0]], np.int32)  # frames 0, 2, 4 sit in different view slots of different chunks


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope='module')
def chunks():
    """The chunk lists (host and device; the device tensors live as long as the module, so the vote plan is built once)."""
    rs = np.random.RandomState(5)
    inds = []
    for n in LENGTHS:
        rest = rs.choice(np.setdiff1d(np.arange(280), [7]), n - 1, replace=False)
        inds.append(rs.permutation(np.concatenate([[7], rest])).astype(np.int64))   # point 7 lies in all four, 280 .. 299 in none
    count = np.bincount(np.concatenate(inds), minlength=N_PTS)
    assert count[7] == 4 and (count == 0).sum() >= 20 and (count == 1).any() and (count == 2).any()
    base, at = [], 0
    for gap, n in zip(GAPS, LENGTHS):
        at += gap
        base.append(at)
        at += n
    return dict(host=inds, dev=[t(i) for i in inds], knn_base=base, rows=at + GAPS[-1], count=count)


def make_knn(chunks, k, seed):
    rs = np.random.RandomState(seed)
    knn = np.full((chunks['rows'], k), 1 << 40, np.int64)  # far out of range wherever no chunk has a row
    knn[::2] = -(1 << 40)
    for b, n in zip(chunks['knn_base'], LENGTHS):
        rows = rs.randint(0, NV * H * W, (n, k)).astype(np.int64)
        rows[rs.rand(n, k) < 0.1] = -1
        knn[b:b + n] = rows
    knn[chunks['knn_base'][2] + 5] = -1            # a row without any neighbour
    knn[chunks['knn_base'][0], 0] = NV * H * W - 1  # the last pixel of the last view
    return knn


def make_store(logical, layout):
    """logical (U,C,h,w) float32 -> a device tensor of that shape and those values in the memory `layout`."""
    x = torch.from_numpy(logical)
    if layout == 'nchw':
        return x.to(DEV).contiguous()
    if layout == 'channels_last':
        out = torch.empty((U, H, W, x.size(1)), dtype=torch.float32, device=DEV).permute(0, 3, 1, 2)
        out.copy_(x)
        assert out.data_ptr() % 16 == 0 and out.stride(1) == 1 and out.stride(3) == x.size(1)
        return out
    buf = torch.empty(x.numel() + 1, dtype=torch.float32, device=DEV)   # channels-last rows from a base that is only 4-byte aligned
    out = buf[1:].view(U, H, W, x.size(1)).permute(0, 3, 1, 2)
    out.copy_(x)
    assert out.data_ptr() % 16 == 4
    return out


@pytest.mark.parametrize('layout', ['channels_last', 'nchw', 'channels_last_unaligned'])
@pytest.mark.parametrize('C', [20, 1, 13, 64])
@pytest.mark.parametrize('k', [1, 3, 5, 8])
def test_kernel_equals_the_oracle_bit_for_bit(chunks, k, C, layout):
    import mvpnet_amd.ops as ops
    from mvpnet_amd import _lib as L
    rs = np.random.RandomState(100 * k + C)
    logical = (rs.standard_normal((U, C, H, W)) * 10 ** rs.uniform(-3, 3, (U, C, H, W))).astype(np.float32)
    knn = make_knn(chunks, k, seed=k)
    etotal, ecount = LO.lift_vote_f32(np.ascontiguousarray(logical.reshape(U, C, H * W).transpose(0, 2, 1)), VIEW_FRAME, knn, chunks['knn_base'],
                                      chunks['host'], N_PTS)
    assert np.array_equal(ecount, chunks['count'])
    store, knn_t = make_store(logical, layout), t(knn)
    total, count = ops.lift_vote(store, t(VIEW_FRAME), knn_t, chunks['knn_base'], chunks['dev'], N_PTS)
    assert total.dtype == torch.float32 and count.dtype == torch.int32
    got = total.cpu().numpy()
    assert np.array_equal(count.cpu().numpy(), ecount)
    assert np.array_equal(got.view(np.uint32), etotal.view(np.uint32)), 'largest difference %g' % float(np.abs(got - etotal).max())
    again, _ = ops.lift_vote(store, t(VIEW_FRAME).long(), knn_t, chunks['knn_base'], chunks['dev'], N_PTS)   # (an int64 frame table is converted)
    assert torch.equal(again.view(torch.int32), total.view(torch.int32)), 'the same bits every run'
    mean = torch.empty_like(total)
    label = torch.empty(N_PTS, dtype=torch.int64, device=DEV)
    L.call('mvp_vote_finish_f32', total, L.ptr(total), L.ptr(count), N_PTS, C, L.ptr(mean), L.ptr(label))
    emean, elabel = LO.finish(etotal, ecount)
    assert np.array_equal(mean.cpu().numpy().view(np.uint32), emean.view(np.uint32)) and np.array_equal(label.cpu().numpy(), elabel)
    none = ecount == 0
    assert (got[none] == 0).all() and (label.cpu().numpy()[none] == C).all()


def test_wrapper_refuses_bad_arguments_before_the_launch(chunks):
    import mvpnet_amd.ops as ops
    store, vf, knn = torch.zeros(U, 20, H, W, device=DEV), t(VIEW_FRAME), t(make_knn(chunks, 3, 0))
    base, inds = chunks['knn_base'], chunks['dev']
    bad = [lambda: ops.lift_vote(store.double(), vf, knn, base, inds, N_PTS),
           lambda: ops.lift_vote(torch.zeros(U, 65, H, W, device=DEV), vf, knn, base, inds, N_PTS),
           lambda: ops.lift_vote(store[:, :, ::2, :], vf, knn, base, inds, N_PTS),          # pixels at two strides
           lambda: ops.lift_vote(store, vf, knn.int(), base, inds, N_PTS),
           lambda: ops.lift_vote(store, vf, torch.zeros(knn.size(0), 9, dtype=torch.int64, device=DEV), base, inds, N_PTS),
           lambda: ops.lift_vote(store, vf[:3], knn, base, inds, N_PTS),
           lambda: ops.lift_vote(store, vf, knn, base[:3], inds, N_PTS),
           lambda: ops.lift_vote(store, vf, knn, base[:3] + [knn.size(0) - 63], inds, N_PTS),  # the last chunk would read past knn
           lambda: ops.lift_vote(store, vf, knn, [-1] + base[1:], inds, N_PTS),
           lambda: ops.lift_vote(store.cpu(), vf, knn, base, inds, N_PTS)]
    for f in bad:
        with pytest.raises(RuntimeError):
            f()


def test_kernel_runs_inside_a_captured_graph(chunks):
    """The entry point only enqueues one launch on the given stream: captured once, replayed on other logits through the same buffers."""
    from mvpnet_amd import _lib as L
    from mvpnet_amd import dist as D
    k, C = 3, 20
    rs = np.random.RandomState(9)
    knn = make_knn(chunks, k, seed=9)
    store = torch.zeros((U, H, W, C), device=DEV).permute(0, 3, 1, 2)
    vf, knn_t, base = t(VIEW_FRAME), t(knn), t(np.array(chunks['knn_base'], np.int64))
    plan = D._vote_plan(chunks['dev'], N_PTS, DEV)
    total = torch.full((N_PTS, C), -1.0, device=DEV)
    count = torch.full((N_PTS,), -1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        L.call('mvp_lift_vote_f32', store, L.ptr(store), store.stride(0), store.stride(3), store.stride(1), U, H * W, C, L.ptr(vf), NV, L.ptr(knn_t), k,
               L.ptr(base), L.ptr(plan['chunk_offsets']), len(LENGTHS), L.ptr(plan['pt_offsets']), L.ptr(plan['pt_slots']), N_PTS, L.ptr(total),
               L.ptr(count))
    for rep in range(2):
        logical = rs.standard_normal((U, C, H, W)).astype(np.float32)
        store.copy_(torch.from_numpy(logical))
        total.fill_(-1.0)
        count.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        etotal, ecount = LO.lift_vote_f32(np.ascontiguousarray(logical.reshape(U, C, H * W).transpose(0, 2, 1)), VIEW_FRAME, knn, chunks['knn_base'],
                                          chunks['host'], N_PTS)
        assert np.array_equal(total.cpu().numpy().view(np.uint32), etotal.view(np.uint32)) and np.array_equal(count.cpu().numpy(), ecount)
