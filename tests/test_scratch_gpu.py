"""-m gpu: the plumbing the non-training operators of ``ops`` share -- one grow-only workspace per operator and device
with a stream hand-over (``ops._scratch``), the state a ``*_launch`` returns, and the named streams.  The smallest
shapes the operators take; nothing here tries to provoke a race: the hand-over is asserted through the cache's own record
of the last stream and event."""
import numpy as np
import pytest
import torch

from neurips18_hierchical_image_manipulation_amd import ops
from neurips18_hierchical_image_manipulation_amd._cabi import lib

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _entries(tag):
    return [s for (t, dev), s in ops._SCRATCH.items() if t == tag and dev == torch.cuda.current_device()]


def _solve(canvas, H, W, seed):
    g = np.random.default_rng(seed)
    P = torch.from_numpy(g.random((1, 3, H, W), dtype=np.float32)).to(DEV)
    region = torch.ones((H, W), dtype=torch.uint8, device=DEV)
    u, status, resid = ops.region_poisson_solve(canvas, 3, 2, P, region, max_iter=4)
    return u.cpu(), status.cpu(), resid.cpu()


def test_one_buffer_per_operator_that_grows_and_never_shrinks():
    tag = 'region_poisson_solve'
    torch.cuda.synchronize()
    ops._SCRATCH.pop((tag, torch.cuda.current_device()), None)     # whatever an earlier test left: start from nothing
    canvas = torch.from_numpy(np.random.default_rng(0).random((1, 3, 16, 16), dtype=np.float32)).to(DEV)
    small, large = int(lib.him_region_poisson_ws(8, 8)), int(lib.him_region_poisson_ws(12, 10))
    assert 0 < small < large
    first = _solve(canvas, 8, 8, 1)
    (s,) = _entries(tag)
    assert small <= s.buf.numel() < large and s.buf.dtype == torch.uint8 and s.buf.data_ptr() % 16 == 0
    _solve(canvas, 12, 10, 2)
    (s2,) = _entries(tag)
    assert s2 is s and s.buf.numel() >= large
    ptr = s.buf.data_ptr()
    third = _solve(canvas, 8, 8, 1)
    (s3,) = _entries(tag)
    assert s3 is s and s.buf.data_ptr() == ptr and s.buf.numel() >= large
    for a, b in zip(first, third):
        assert torch.equal(a, b)


def test_hand_over_between_two_streams(monkeypatch):
    g = np.random.default_rng(7)
    x1, y1, x2, y2 = (torch.from_numpy(g.random((1, 1, 16, 16), dtype=np.float32)).to(DEV) for _ in range(4))
    kw = dict(scale=255.0, offset=0.0, quantize=True, data_range=255.0)
    alone1, alone2 = ops.image_metrics(x1, y1, **kw)[0].cpu(), ops.image_metrics(x2, y2, **kw)[0].cpu()
    assert not torch.equal(alone1, alone2)
    torch.cuda.synchronize()
    (s,) = _entries('image_metrics')
    assert s.stream == torch.cuda.current_stream()
    waits = []
    wait_event = torch.cuda.Stream.wait_event
    monkeypatch.setattr(torch.cuda.Stream, 'wait_event', lambda self, ev: (waits.append((self, ev)), wait_event(self, ev))[1])
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(A):
        r1 = ops.image_metrics(x1, y1, **kw)[0]
        assert s.stream == A
    with torch.cuda.stream(B):                                     # no synchronisation in between
        r2 = ops.image_metrics(x2, y2, **kw)[0]
    monkeypatch.undo()
    assert _entries('image_metrics') == [s] and s.stream == B and s.stream != A
    # A waited for the event behind the calls on the default stream, B for the one behind the call on A
    assert len(waits) == 2 and waits[0][0] == A and waits[1][0] == B and all(ev is s.event for _, ev in waits)
    A.synchronize()
    B.synchronize()
    assert s.event.query()
    assert torch.equal(r1.cpu(), alone1) and torch.equal(r2.cpu(), alone2)


def test_the_five_named_streams_are_distinct_and_created_once():
    dev = torch.device('cuda', torch.cuda.current_device())
    getters = (ops._side_stream, ops._opt_stream, ops._vgg_stream, ops._real_stream, ops._d_opt_stream)
    streams = [get(dev) for get in getters]
    assert all(isinstance(s, torch.cuda.Stream) and s.device == dev for s in streams)
    assert len(set(id(s) for s in streams)) == 5
    for get, s in zip(getters, streams):
        assert get(dev) is s


def test_launch_state_is_read_by_subscript():
    label = torch.zeros((2, 8, 8), dtype=torch.uint8, device=DEV)
    label[0, 1:3, 1:3] = 5
    label[0, 5:7, 4:8] = 5
    label[1, 2:6, 2:6] = 5
    inst, counts, st = ops.label_instances_launch(label, things=(5,))
    assert tuple(st['out'].shape) == (2, 2) and st['out'].dtype == torch.int32 and st['out'].is_cuda
    assert tuple(st['host'].shape) == (2, 2) and st['host'].is_pinned()
    launched = counts.cpu().tolist()
    inst2, host_counts = ops.label_instances(label, things=(5,))
    assert launched == host_counts.tolist() == [2, 1] and st['out'][:, 0].cpu().tolist() == [2, 1]
    assert torch.equal(inst, inst2)


def test_a_workspace_of_zero_bytes_is_still_a_pointer():
    tag = 'test_scratch_gpu: zero bytes'
    with ops._scratch(tag, 0) as ws:
        assert ws.numel() >= 1 and ws.data_ptr() != 0 and ws.data_ptr() % 16 == 0
    (s,) = _entries(tag)
    assert s.stream == torch.cuda.current_stream()
    del ops._SCRATCH[tag, torch.cuda.current_device()]
    with ops._scratch('ade_decode', lib.him_ade_decode_workspace()) as ws:
        assert ws.data_ptr() != 0 and ws.numel() >= max(int(lib.him_ade_decode_workspace()), 1)
