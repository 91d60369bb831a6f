"""The instrumented allocator of the scratch-state tests (tests/scratch_arena.py) on CPU tensors: what it hands out, what it replays and
what its guard check reports.  No project kernel runs here."""
import types

import pytest
import torch

import scratch_arena as SA
from scratch_arena import Arena, ArenaError, GUARD_BYTE


def _cpu_arena(**kw):
    return Arena(device_type='cpu', **kw)


def test_proxy_forwards_everything_but_device_empty():
    px = Arena().proxy()
    assert px.Tensor is torch.Tensor and px.int32 is torch.int32 and px.cuda is torch.cuda and px.no_grad is torch.no_grad
    assert px.zeros is torch.zeros and px.autograd.Function is torch.autograd.Function
    assert isinstance(px.ones(3), px.Tensor)
    with pytest.raises(AttributeError):
        px.no_such_attribute


def test_non_device_requests_pass_through():
    arena = Arena()                                                  # serves 'cuda' requests only
    px = arena.proxy()
    a = px.empty(5, dtype=torch.int32)
    b = px.empty((2, 3), dtype=torch.float32, device='cpu')
    c = px.empty_like(b)
    m = px.empty(7, device='meta')
    assert a.shape == (5,) and b.shape == (2, 3) and c.shape == (2, 3) and c.dtype == torch.float32 and m.device.type == 'meta'
    assert arena.blocks == [] and arena.sequence() == []
    cpu = _cpu_arena()
    assert cpu.proxy().empty(7, device='meta').device.type == 'meta' and cpu.proxy().empty(3, device='cpu', pin_memory=False).shape == (3,)
    assert len(cpu.blocks) == 1                                      # (the meta request went through, the cpu one is the arena's)


@pytest.mark.parametrize('shape, dtype', [((1,), torch.uint8), ((13,), torch.uint8), ((3, 5), torch.float32), ((27, 17), torch.int32),
                                          ((0,), torch.int64), ((0, 4), torch.int32), ((1025,), torch.int16), ((4097,), torch.float64)])
def test_payload_is_exact_aligned_zero_and_guarded(shape, dtype):
    arena = _cpu_arena()
    px = arena.proxy()
    t = px.empty(shape, dtype=dtype, device='cpu') if len(shape) > 1 else px.empty(*shape, dtype=dtype, device='cpu')
    blk = arena.blocks[0]
    nbytes = t.numel() * t.element_size()
    assert t.shape == shape and t.dtype == dtype and t.is_contiguous()
    assert blk.nbytes == nbytes and arena.sequence() == [(nbytes, dtype)]
    assert (blk.buf.data_ptr() + blk.lead) % 512 == 0
    assert nbytes == 0 or t.data_ptr() == blk.buf.data_ptr() + blk.lead          # (an empty tensor has no address)
    assert not t.any()                                               # fresh: zeros
    (_, before), (_, after) = blk.guards()
    assert len(before) >= max(nbytes, 4096) and len(after) >= max(nbytes, 4096)
    assert len(before) + nbytes + len(after) == len(blk.buf)          # nothing between payload and guards: no rounding up
    assert (before == GUARD_BYTE).all() and (after == GUARD_BYTE).all()
    arena.check()
    like = px.empty_like(t)
    assert like.shape == shape and like.dtype == dtype and len(arena.blocks) == 2 and like.data_ptr() % 512 == 0 and arena.blocks[1].nbytes == nbytes


def test_stale_replay_serves_the_same_memory_with_its_bytes():
    rec = _cpu_arena()
    px = rec.proxy()
    a = px.empty(10, dtype=torch.int32, device='cpu')
    b = px.empty((4, 4), dtype=torch.float32, device='cpu')
    a.copy_(torch.arange(10, dtype=torch.int32))
    b.fill_(2.5)
    rec.check()
    stale = rec.replay()
    sx = stale.proxy()
    a2 = sx.empty(10, dtype=torch.int32, device='cpu')
    b2 = sx.empty(16, dtype=torch.float32, device='cpu')             # same bytes and dtype, another shape: the same block
    assert a2.data_ptr() == a.data_ptr() and b2.data_ptr() == b.data_ptr()
    assert a2.tolist() == list(range(10)) and b2.shape == (16,) and (b2 == 2.5).all()
    stale.finish()
    stale.check()
    assert stale.stats()[:2] == (2, 2) and rec.stats()[:2] == (2, 0) and stale.served_fresh == []


def _caller_x(px, n):
    return px.empty(n, dtype=torch.int32, device='cpu')


def test_sequence_mismatch_is_reported_and_named_callers_are_served_fresh():
    rec = _cpu_arena()
    _caller_x(rec.proxy(), 10).fill_(7)
    rec.proxy().empty(3, dtype=torch.uint8, device='cpu')
    with pytest.raises(ArenaError, match=r'request 0 from _caller_x\(\) is 44 bytes.*recorded run asked for 40 bytes') as e:
        _caller_x(rec.replay().proxy(), 11)
    assert 'recorded: 0:40B/int32 1:3B/uint8' in str(e.value) and 'this run: 0:44B/int32' in str(e.value)
    with pytest.raises(ArenaError, match='request 0'):              # same bytes, another dtype
        rec.replay().proxy().empty(40, dtype=torch.uint8, device='cpu')
    stale = rec.replay(fresh_ok=('_caller_x',))
    t = _caller_x(stale.proxy(), 11)
    assert not t.any() and stale.served_fresh == [(0, '_caller_x', (44, torch.int32), (40, torch.int32))]
    with pytest.raises(ArenaError, match='1 requests, the recorded run made 2'):
        stale.finish()
    u = stale.proxy().empty(3, dtype=torch.uint8, device='cpu')       # the next request is replayed again
    stale.finish()
    assert stale.stats()[:2] == (2, 1) and u.data_ptr() == rec.blocks[1].payload().data_ptr()
    with pytest.raises(ArenaError, match='nothing more'):
        stale.proxy().empty(3, dtype=torch.uint8, device='cpu')


@pytest.mark.parametrize('side', ['before', 'after'])
def test_a_write_one_element_outside_the_payload_fails_check(side):
    arena = _cpu_arena()
    px = arena.proxy()
    px.empty(100, dtype=torch.float32, device='cpu')
    t = px.empty((9, 3), dtype=torch.int32, device='cpu')
    px.empty(5, dtype=torch.uint8, device='cpu')
    arena.check()
    blk = arena.blocks[1]
    whole = blk.buf[blk.lead - 4:blk.lead + blk.nbytes + 4].view(torch.int32)      # the payload with one element on either side
    assert whole[1:-1].data_ptr() == t.data_ptr()
    whole[0 if side == 'before' else -1] = 0
    want = r'allocation 1 \(108 bytes of torch.int32.*' + (r'before the payload: 4 bytes, the first at offset -4' if side == 'before'
                                                          else r'after the payload: 4 bytes, the first at offset 0')
    with pytest.raises(ArenaError, match=want):
        arena.check()
    whole[0 if side == 'before' else -1] = int.from_bytes(bytes([GUARD_BYTE] * 4), 'little', signed=True)
    arena.check()


def test_installed_swaps_torch_in_a_module_and_puts_it_back(monkeypatch):
    mod = types.ModuleType('pcgcv2_amd._arena_probe')
    mod.torch = torch
    monkeypatch.setitem(SA.sys.modules, 'pcgcv2_amd._arena_probe', mod)
    monkeypatch.setattr(SA, 'product_modules', lambda: [mod])
    arena = _cpu_arena()
    with SA.installed(arena):
        assert mod.torch is not torch and mod.torch.float32 is torch.float32
        mod.torch.empty(4, device='cpu')
    assert mod.torch is torch and len(arena.blocks) == 1
