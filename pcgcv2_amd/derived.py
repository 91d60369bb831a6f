"""Derived copies of the weights (MFMA fragment tables, packed entropy parameters): ONE stamp and ONE way to publish an entry.

The hot path does not read `kernel` directly but a re-laid-out copy cached on the module.  A cache entry is valid while the parameter
tensors it was built from are the same tensors with the same values; this module decides that ("cache contract"):

  stamp(params)     (data_ptr, _version) per tensor: one tuple compare per call.  Every in-place update that goes through autograd's
                    version counter (optimizer steps, `p.copy_`, `p.mul_`, load_state_dict) changes `_version`; every replacement of
                    the tensor (`p.data = w`, vector_to_parameters, load_state_dict(assign=True), `.half().float()`, `.to()`) changes
                    `data_ptr` — PROVIDED the old block cannot have been freed and handed back by the caching allocator at the same
                    address.  An Entry therefore holds an alias (`p.detach()`) of every tensor it was built from: while the entry
                    lives, the old storage lives, and no new tensor can sit at its address.  Cost: one stale copy of a layer's
                    weights between a replacement and the next rebuild.
  optimizer epoch   a fused optimizer (`torch.optim.Adam(..., fused=True)`) updates the parameters in one multi-tensor kernel that bumps no
                    version counter (seen on torch 2.10: `_version` is the same before and after `step()`).  Every stamp therefore
                    starts with a process-wide epoch that a global optimizer post-step hook advances: after ANY `torch.optim` step,
                    every derived copy is rebuilt on next use — which an optimizer step means anyway.
  weights_changed   writes through `.data` (`p.data.mul_(s)`, `p.data.copy_(w)`: weight clamping, EMA) change neither the pointer nor
                    the version; nothing short of a checksum per layer per call could see them.  The contract is ONE explicit call
                    after such writes, `module.weights_changed()`, on a PCCModel or any module below it: it drops every derived copy
                    in that subtree.
  publish / order   an entry is built by torch ops enqueued on the builder's current stream.  It is stored together with an event
                    recorded behind the build; a consumer that finds the entry waits for that event on its own stream (a no-op on
                    the builder's) before it launches, and records its stream on the table's storage, so no stream can read a
                    half-written table or one whose block was handed out again.  Once the event has completed it
                    is dropped: a warm entry costs the tuple compare and one `is None`.  Two threads that miss at once may both
                    build; each stores only a complete (stamp, alias, value, event) record, by one dict assignment.

What this does NOT order: an update of the weights while another stream still has kernels in flight that read them.  That is the
caller's to order, for the derived copies exactly as for the parameters themselves."""
import torch
from torch.optim.optimizer import register_optimizer_step_post_hook

_EPOCH = [0]


def _optimizer_stepped(optimizer, args, kwargs):
    _EPOCH[0] += 1


register_optimizer_step_post_hook(_optimizer_stepped)


def stamp(params, device=False):
    """optimizer epoch, then identity + version of each parameter tensor -> tuple to compare; device=True adds each tensor's device (a
    module whose derived copies live on another device than its parameters)"""
    if device:
        return (_EPOCH[0],) + tuple((p.data_ptr(), p._version, p.device) for p in params)
    return (_EPOCH[0],) + tuple((p.data_ptr(), p._version) for p in params)


class Entry:
    """one published derived copy: stamp it is valid for, aliases that pin the storages the stamp names, the value, and — until it
    has completed — the event recorded behind the build"""
    __slots__ = ('stamp', 'alias', 'value', 'event', 'stream')

    def __init__(self, stamp, alias, value, event, stream):
        self.stamp, self.alias, self.value, self.event, self.stream = stamp, alias, value, event, stream

    def __reduce__(self):
        """a copied or pickled module (copy.deepcopy, torch.save of a module) carries no derived copy: an entry that matches no stamp"""
        return (Entry, (None, (), None, None, None))

    def __deepcopy__(self, memo):
        return Entry(None, (), None, None, None)


def publish(stamp_, params, build, device=None):
    """build() on the current stream of `device` (default: the first parameter's) -> a complete Entry"""
    alias = tuple(p.detach() for p in params)
    value = build()
    device = params[0].device if device is None else torch.device(device)
    event = stream = None
    if device.type == 'cuda':
        stream = torch.cuda.current_stream(device)
        event = torch.cuda.Event()
        event.record(stream)
    return Entry(stamp_, alias, value, event, stream)


def order(entry):
    """make the current stream wait for the entry's build (nothing to do once the build has completed, or on the builder's stream)"""
    ev = entry.event
    if ev is None:
        return
    if ev.query():
        entry.event = None
        return
    cur = torch.cuda.current_stream(entry.stream.device)
    if cur != entry.stream:
        cur.wait_event(ev)
        # the value was allocated from the builder stream's pool: tell the allocator that this stream reads it too, so that a block freed
        # by a rebuild (or by a second builder that stores over this entry) is not handed out again while this stream's kernels are in flight
        for t in (entry.value if isinstance(entry.value, tuple) else (entry.value,)):
            if torch.is_tensor(t):
                t.record_stream(cur)


def fetch(slots, name, params, build):
    """the derived copy `name` of `params` from the dict `slots` (a module's own), rebuilt when the stamp differs"""
    s = stamp(params)
    e = slots.get(name)
    if e is None or e.stamp != s:
        e = slots[name] = publish(s, params, build)
    elif e.event is not None:
        order(e)
    return e.value


def weights_changed(module):
    """The explicit call of the cache contract: after writes that the stamp cannot see (through `.data`), drop every derived copy held
    by `module` and the modules below it.  Cheap (a few dict pops); the next forward rebuilds what it needs."""
    for m in module.modules():
        drop = getattr(m, '_drop_derived', None)
        if drop is not None:
            drop()
