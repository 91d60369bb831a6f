"""An instrumented allocator for the tests of scratch state (test_scratch_state_cpu.py, test_scratch_state_device.py).

The wrappers in pcgcv2_amd allocate every workspace and every output with torch.empty and rely on native clears (hipMemsetAsync,
k_hash_clear) of exactly the parts the kernels need.  A test process mostly receives zeroed memory, where a missing or short clear has no
effect, and nothing ever looks at the bytes around a buffer.  An Arena stands in for `torch` inside a product module

    monkeypatch.setattr(ops, 'torch', arena.proxy())

and serves every device torch.empty / torch.empty_like from memory it owns, laid out [guard | payload | guard]:

  * the payload has exactly the requested bytes (no rounding up) and starts at a multiple of 512 bytes (the caching allocator's
    granularity: kernels that choose a path by alignment take the path they take in production);
  * each guard is at least as large as the payload and at least 4 KiB and holds GUARD_BYTE: an index doubled by a stale counter still
    lands inside the arena's own allocation and shows as a damaged guard, not as a fault;
  * mode 'fresh': the payload is zero-filled (what a new process sees); `arena.replay()` gives the 'stale' arena, which serves its i-th
    request from the block the i-th request of the recorded run used, NOT refilled: it holds that run's final descriptors, tickets, hash
    slots and partial sums, all legal for the shape and wrong for the data.  Payloads are never pattern-filled: many hold indices.

The stale run's sequence of (bytes, dtype) must equal the recorded one.  A request that differs is an error (both sequences are printed)
unless the function that made it is named in `fresh_ok` (allocations whose size depends on the data): that one is served fresh and listed
in `arena.served_fresh`.  `arena.check()` synchronises and verifies every guard byte."""
import sys

import torch

GUARD_BYTE = 0xA5
ALIGN = 512
MIN_GUARD = 4096


class ArenaError(AssertionError):
    pass


class _Block:
    __slots__ = ('index', 'buf', 'lead', 'nbytes', 'dtype', 'shape', 'caller', 'replayed')

    def __init__(self, index, nbytes, dtype, shape, device, caller):
        guard = (max(nbytes, MIN_GUARD) + ALIGN - 1) // ALIGN * ALIGN
        self.buf = torch.full((ALIGN + 2 * guard + nbytes,), GUARD_BYTE, dtype=torch.uint8, device=device)
        self.lead = guard + (-(self.buf.data_ptr() + guard)) % ALIGN                   # the payload's ADDRESS is a multiple of ALIGN
        self.index, self.nbytes, self.dtype, self.shape, self.caller, self.replayed = index, nbytes, dtype, tuple(shape), caller, False
        self.buf[self.lead:self.lead + nbytes].zero_()

    def payload(self, shape=None):
        return self.buf[self.lead:self.lead + self.nbytes].view(self.dtype).view(self.shape if shape is None else tuple(shape))

    def guards(self):
        return (('before', self.buf[:self.lead]), ('after', self.buf[self.lead + self.nbytes:]))

    def key(self):
        return (self.nbytes, self.dtype)


def _fmt(seq):
    return ' '.join(f'{i}:{n}B/{str(d).replace("torch.", "")}' for i, (n, d) in enumerate(seq))


class _Proxy:
    """every attribute of torch, except empty / empty_like for the arena's device"""

    def __init__(self, arena):
        object.__setattr__(self, '_arena', arena)

    def __getattr__(self, name):
        return getattr(torch, name)

    def __setattr__(self, name, value):
        setattr(torch, name, value)

    def empty(self, *size, **kw):
        return self._arena._empty(size, kw)

    def empty_like(self, t, **kw):
        return self._arena._empty_like(t, kw)


class Arena:
    def __init__(self, device_type='cuda', recorded=None, fresh_ok=()):
        """device_type: the torch device type whose requests the arena serves (the CPU tests of the arena itself use 'cpu');
        recorded: the blocks of an earlier run (use replay()); fresh_ok: names of the functions whose requests may differ from it"""
        self.device_type = device_type
        self.mode = 'fresh' if recorded is None else 'stale'
        self.recorded = recorded
        self.fresh_ok = tuple(fresh_ok)
        self.blocks = []
        self.served_fresh = []                      # [(index, caller, (bytes, dtype) asked, (bytes, dtype) recorded or None)]

    # ---------------------------------------------------------------------------------------- the stand-in
    def proxy(self):
        return _Proxy(self)

    def replay(self, fresh_ok=()):
        """-> the stale arena over this (finished, checked) run's blocks"""
        return Arena(self.device_type, recorded=list(self.blocks), fresh_ok=fresh_ok)

    def _is_ours(self, device, kw):
        if kw.get('pin_memory') or kw.get('out') is not None or kw.get('requires_grad'):
            return False
        layout = kw.get('layout')
        if layout is not None and layout != torch.strided:
            return False
        return device is not None and torch.device(device).type == self.device_type

    def _empty(self, size, kw):
        if not self._is_ours(kw.get('device'), kw):
            return torch.empty(*size, **kw)
        if 'size' in kw:
            size = (kw['size'],)
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(int(s) for s in size)
        dtype = kw.get('dtype') or torch.get_default_dtype()
        return self._serve(shape, dtype, torch.device(kw['device']))

    def _empty_like(self, t, kw):
        device = kw.get('device', t.device)
        if not self._is_ours(device, kw):
            return torch.empty_like(t, **kw)
        return self._serve(tuple(t.shape), kw.get('dtype') or t.dtype, torch.device(device))

    def _serve(self, shape, dtype, device):
        numel = 1
        for s in shape:
            numel *= int(s)
        nbytes = numel * torch.empty((), dtype=dtype).element_size()
        caller = sys._getframe(3).f_code.co_name                        # _serve <- _empty <- proxy.empty <- the product function
        i = len(self.blocks)
        if self.mode == 'stale':
            old = self.recorded[i] if i < len(self.recorded) else None
            if old is not None and old.key() == (nbytes, dtype) and old.buf.device.type == device.type:
                old_view = _Block.__new__(_Block)
                for s in _Block.__slots__:
                    setattr(old_view, s, getattr(old, s))
                old_view.shape, old_view.caller, old_view.replayed = tuple(shape), caller, True
                self.blocks.append(old_view)
                return old_view.payload()
            if caller not in self.fresh_ok:
                asked = [b.key() for b in self.blocks] + [(nbytes, dtype)]
                raise ArenaError(f'stale replay: request {i} from {caller}() is {nbytes} bytes of {dtype}, the recorded run asked for '
                                 f'{"nothing more" if old is None else f"{old.nbytes} bytes of {old.dtype} (from {old.caller}())"}\n'
                                 f'  recorded: {_fmt([b.key() for b in self.recorded])}\n  this run: {_fmt(asked)}')
            self.served_fresh.append((i, caller, (nbytes, dtype), None if old is None else old.key()))
        block = _Block(i, nbytes, dtype, shape, device, caller)
        self.blocks.append(block)
        return block.payload()

    # ---------------------------------------------------------------------------------------- after the run
    def sequence(self):
        return [b.key() for b in self.blocks]

    def finish(self):
        """a stale run must have made every request of the recorded run"""
        if self.mode == 'stale' and len(self.blocks) != len(self.recorded):
            raise ArenaError(f'stale replay: {len(self.blocks)} requests, the recorded run made {len(self.recorded)}\n'
                             f'  recorded: {_fmt([b.key() for b in self.recorded])}\n  this run: {_fmt(self.sequence())}')

    def check(self):
        """synchronise, then every guard byte must be intact; ArenaError names the allocation, the side and the first damaged offset"""
        if self.device_type == 'cuda':
            torch.cuda.synchronize()
        flags = [(g == GUARD_BYTE).all() for b in self.blocks for _, g in b.guards()]
        if not flags or bool(torch.stack(flags).all()):
            return
        for b in self.blocks:
            for side, g in b.guards():
                bad = (g != GUARD_BYTE).nonzero()
                if len(bad):
                    first = int(bad[0])
                    at = first - len(g) if side == 'before' else first      # relative to the payload: negative = before its first byte
                    raise ArenaError(f'guard damaged: allocation {b.index} ({b.nbytes} bytes of {b.dtype}, shape {b.shape}, from {b.caller}()), '
                                     f'{side} the payload: {len(bad)} bytes, the first at offset {at} from the payload\'s '
                                     f'{"start" if side == "before" else "end"} (value {int(g[first])})')

    def stats(self):
        """(allocations, replayed allocations, guard bytes)"""
        return (len(self.blocks), sum(b.replayed for b in self.blocks), sum(len(g) for b in self.blocks for _, g in b.guards()))


def product_modules():
    """every module of the package that holds `torch` (all of them allocate through it, or may one day)"""
    import importlib
    for name in ('ops', 'sparse', 'nn', 'autoencoder', 'grad', 'loss', 'entropy_model', 'pc_error', 'attributes', 'lossless', 'coder',
                 'occupancy_model', 'pcc_model', 'derived', 'data_loader', 'generate_dataset', 'estimate_normals', 'recolour'):
        importlib.import_module('pcgcv2_amd.' + name)
    return [m for n, m in sorted(sys.modules.items()) if n.startswith('pcgcv2_amd.') and m is not None and getattr(m, '__dict__', {}).get('torch') is torch]


class installed:
    """with installed(arena): ...  — the arena's proxy as `torch` of every product module, the real one put back on exit"""

    def __init__(self, arena):
        self.arena = arena

    def __enter__(self):
        self.mods = product_modules()
        p = self.arena.proxy()
        for m in self.mods:
            m.__dict__['torch'] = p
        return self.arena

    def __exit__(self, *exc):
        for m in self.mods:
            m.__dict__['torch'] = torch
        return False
