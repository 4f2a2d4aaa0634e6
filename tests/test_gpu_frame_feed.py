"""The frame feed on the GPU (include/sings_feed.h, csrc/sg_feed.hip, sings_amd/frame_feed.py) against its numpy twins: integers and
bit patterns only, no tolerance anywhere.

Expand: three frames that between them hold every byte value in every channel, at sizes that take the 16-byte path (H*W a multiple
of 4: 16 x 64, and 33 x 130 with more than one workgroup per frame and a ragged last one) and the one-pixel path (1 x 1, 5 x 7), K of
1, 3 and 16 with repeated and reversed indices, and indices -1 and F.  Draw: every (F, K) pair for enough calls to cover three epochs
-- K = 3 and 16 straddle epoch boundaries at F = 5, 16, 257, and at F = 1 and 2 one call spans several epochs."""
import numpy as np
import pytest
import torch

from sings_amd import frame_feed as ff

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _store(F, H, W, seed=0):
    """Every byte value in every channel where the frames have room for it (F*H*W >= 256), random bytes elsewhere."""
    rs = np.random.RandomState(seed)
    data = rs.randint(0, 256, (F, H, W, 4)).astype(np.uint8)
    flat = data.reshape(-1, 4)
    n = min(256, flat.shape[0])
    for ch in range(4):
        flat[rs.permutation(flat.shape[0])[:n], ch] = np.arange(n, dtype=np.uint8) if n == 256 else rs.randint(0, 256, n)
    return data, ff.FrameStore(data[..., :3].copy(), data[..., 3].copy(), device=DEV)


def _expected(data, idx):
    table = ff.value_table()
    sel = data[np.clip(np.asarray(idx), 0, data.shape[0] - 1)]
    return table[sel[..., :3]].transpose(0, 3, 1, 2), table[sel[..., 3]]


@pytest.mark.parametrize("H, W", [(1, 1), (5, 7), (16, 64), (33, 130)])
def test_expand_is_the_table_of_the_stored_bytes(H, W):
    F = 3
    data, store = _store(F, H, W, seed=H)
    if F * H * W >= 256:
        assert all(len(np.unique(data[..., ch])) == 256 for ch in range(4))
    assert store.nbytes == F * H * W * 4 and tuple(store.data.shape) == (F, H, W, 4)
    assert np.array_equal(store.data.cpu().numpy(), data)
    for idx in ([1], [2, 0, 2], [2, 1, 0, 0, 1, 2, 2, 2, 1, 0, 1, 0, 0, 2, 1, 1], [-1, F, 1], [-7, 100000, 0, 2]):
        gt, mask = store.frames(idx)
        torch.cuda.synchronize()
        want_gt, want_mask = _expected(data, idx)
        assert tuple(gt.shape) == (len(idx), 3, H, W) and tuple(mask.shape) == (len(idx), H, W)
        assert np.array_equal(_bits(gt.cpu().numpy()), _bits(want_gt)), (H, W, idx)
        assert np.array_equal(_bits(mask.cpu().numpy()), _bits(want_mask)), (H, W, idx)
    gt, mask = store.frames(list(range(F)) * 7)                           # (21 indices: two launches)
    want_gt, want_mask = _expected(data, list(range(F)) * 7)
    assert np.array_equal(_bits(gt.cpu().numpy()), _bits(want_gt)) and np.array_equal(_bits(mask.cpu().numpy()), _bits(want_mask))


@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("F", [1, 2, 5, 16, 257])
def test_draw_follows_the_twin_over_three_epochs(F, K):
    seed = 1000 * F + K
    data, store = _store(F, 2, 2, seed=F)
    feed = ff.FrameFeed(store, seed=seed, frames_per_step=K)
    calls = -(-3 * F // K) + 1
    want = ff.indices_host(F, seed, 0, calls * K).reshape(calls, K)
    got, bgs, counters = [], [], []
    for _ in range(calls):
        feed.draw()
        got.append(feed.idx.clone()); bgs.append(feed.bg.clone()); counters.append(feed.state.clone())
    torch.cuda.synchronize()
    assert np.array_equal(torch.stack(got).cpu().numpy(), want)
    for n in range(calls):
        assert np.array_equal(_bits(bgs[n].cpu().numpy()), _bits(ff.bg_host(seed, n * K))), n
        c, s, held, last = counters[n].tolist()
        assert (c, s, held, last) == ((n + 1) * K, seed, ((n + 1) * K - 1) // F, n * K), n
    assert feed.counter == calls * K and feed.seed == seed and np.array_equal(feed.last_indices, want[-1])
    assert np.array_equal(feed.order.cpu().numpy(), ff.order_host(F, seed, (calls * K - 1) // F))
    # the expanded frames are the drawn ones
    want_gt, want_mask = _expected(data, want[-1])
    assert np.array_equal(_bits(feed.gt.cpu().numpy()), _bits(want_gt)) and np.array_equal(_bits(feed.mask.cpu().numpy()), _bits(want_mask))


def test_a_feed_without_random_bg_leaves_bg_alone():
    _, store = _store(5, 2, 2)
    feed = ff.FrameFeed(store, seed=3, frames_per_step=2, random_bg=False)
    feed.bg.copy_(torch.tensor([0.25, 0.5, 0.75]))
    feed.draw(); feed.draw()
    assert feed.bg.tolist() == [0.25, 0.5, 0.75] and np.array_equal(feed.last_indices, ff.indices_host(5, 3, 2, 2))


def test_the_largest_store_rebuilds_the_twins_order():
    F = ff.MAX_FRAMES
    store = ff.FrameStore(np.zeros((F, 1, 1, 3), np.uint8), (np.arange(F) % 256).astype(np.uint8).reshape(F, 1, 1), device=DEV)
    feed = ff.FrameFeed(store, seed=7, frames_per_step=16)
    feed.load_state_dict({"seed": 7, "counter": 3 * F + 5})
    feed.draw()
    order = ff.order_host(F, 7, 3)
    assert np.array_equal(feed.order.cpu().numpy(), order)
    assert np.array_equal(feed.last_indices, order[5:21]) and feed.counter == 3 * F + 21
    assert np.array_equal(_bits(feed.mask.cpu().numpy().reshape(-1)), _bits(ff.value_table()[order[5:21] % 256]))


def test_a_captured_draw_replays_the_eager_sequence_and_a_loaded_state_continues_it():
    F, K, seed = 5, 2, 77
    _, store = _store(F, 3, 4)
    n = 2 * F + 1
    eager = ff.FrameFeed(store, seed=seed, frames_per_step=K)
    seq, bgs = [], []
    for _ in range(n):
        eager.draw()
        seq.append(eager.idx.clone()); bgs.append(eager.bg.clone())
    feed = ff.FrameFeed(store, seed=seed, frames_per_step=K)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        feed.draw()                                                      # (a warm-up that is not a step: the state goes back)
    torch.cuda.current_stream().wait_stream(side)
    feed.load_state_dict({"seed": seed, "counter": 0})
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        feed.draw()
    feed.load_state_dict({"seed": seed, "counter": 0})                   # (a capture launches nothing; put back all the same)
    got, got_bg, got_gt = [], [], []
    for _ in range(n):
        graph.replay()
        got.append(feed.idx.clone()); got_bg.append(feed.bg.clone()); got_gt.append(feed.gt.clone())
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(got), torch.stack(seq)) and feed.counter == n * K
    assert np.array_equal(torch.stack(got).cpu().numpy().reshape(-1), ff.indices_host(F, seed, 0, n * K))
    assert np.array_equal(_bits(torch.stack(got_bg).cpu().numpy()), _bits(torch.stack(bgs).cpu().numpy()))
    assert torch.equal(got_gt[-1], store.frames(seq[-1])[0])
    # a checkpoint taken in mid-epoch: a fresh feed continues the sequence where the first one stood
    mid = ff.FrameFeed(store, seed=seed, frames_per_step=K)
    for _ in range(3):
        mid.draw()
    sd = mid.state_dict()
    assert sd == {"seed": seed, "counter": 3 * K}
    resumed = ff.FrameFeed(store, seed=0, frames_per_step=K)
    resumed.load_state_dict(sd)
    assert resumed.state.tolist() == [3 * K, seed, -1, 0]
    for step in range(3, n):
        resumed.draw()
        assert torch.equal(resumed.idx, seq[step]) and torch.equal(resumed.bg, bgs[step]), step


def test_from_float_takes_the_references_floats_and_refuses_others():
    rs = np.random.RandomState(4)
    F, H, W = 2, 9, 11
    rgb_u8 = rs.randint(0, 256, (F, H, W, 3)).astype(np.uint8)
    mask_u8 = (rs.randint(0, 2, (F, H, W)) * 255).astype(np.uint8)
    rgb = (rgb_u8.transpose(0, 3, 1, 2) / 255).astype(np.float32)        # (the reference's cache: img / 255 as fp32, planar)
    mask = (mask_u8 / 255).astype(np.float32)
    store = ff.FrameStore.from_float(torch.from_numpy(rgb), torch.from_numpy(mask), device=DEV)
    assert np.array_equal(store.data.cpu().numpy()[..., :3], rgb_u8) and np.array_equal(store.data.cpu().numpy()[..., 3], mask_u8)
    gt, m = store.frames([0, 1])
    assert np.array_equal(_bits(gt.cpu().numpy()), _bits(rgb)) and np.array_equal(_bits(m.cpu().numpy()), _bits(mask))
    lossy = rgb.copy()
    lossy[1, 2, 3, 4], lossy[0, 0, 0, 0] = 0.3, np.float32(7.0) * np.float32(1.0 / 255.0)
    assert lossy[0, 0, 0, 0] != np.float32(7.0) / np.float32(255.0)
    with pytest.raises(ValueError, match=r"FrameStore.from_float: 2 of \d+ elements"):
        ff.FrameStore.from_float(torch.from_numpy(lossy), torch.from_numpy(mask), device=DEV)
    with pytest.raises(ValueError, match="1 of"):
        ff.FrameStore.from_float(torch.from_numpy(rgb), torch.from_numpy(np.where(np.arange(mask.size).reshape(mask.shape) == 5,
                                                                                   np.float32(np.nan), mask)), device=DEV)
