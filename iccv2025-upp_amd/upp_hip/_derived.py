"""Buffers DERIVED from weights and kept beside them: functional.TRANSPOSED (W^T copies of the data-gradient GEMMs) and ops.PLANES (bf16 plane
images of the split-bf16 kernels) are two instances of the cache below.  Pure torch: how a buffer is made, refilled and batch-refreshed
is handed in by the instance's keeper."""
import contextlib
import weakref

import torch


def any_owner(owner):
    return True


def persistent_owner(owner):          # an nn.Parameter, or a buffer marked by its keeper: a tensor that outlives the step that uses it
    return isinstance(owner, torch.nn.Parameter) or getattr(owner, "_upp_persistent", False)


class Entry:
    """anchor: weak reference to the tensor the entry lives and dies with (the storage owner, as a rule); version: the owner's version
    counter when `derived` was last filled; geom: (shape, stride, storage offset) of the window `derived` was made from; tag: the keeper's."""
    __slots__ = ("anchor", "version", "derived", "geom", "tag")

    def __init__(self, anchor, version, derived, geom, tag=None):
        self.anchor, self.version, self.derived, self.geom, self.tag = weakref.ref(anchor), version, derived, geom, tag

    def __getitem__(self, i):          # (positional access as in the lists these records replace)
        return getattr(self, self.__slots__[i])

    def __setitem__(self, i, value):
        setattr(self, self.__slots__[i], value)

    def owner(self):
        a = self.anchor()
        return a if a is None or a._base is None else a._base

    def view(self):
        """The window as it reads now."""
        return torch.as_strided(self.anchor().detach(), *self.geom)


class DerivedWeights:
    """One derived buffer per weight WINDOW -- key (address, shape, stride); a column window of a parameter shares its version counter.
    `entries`, FROZEN weights: made on first use (the eager warm-up of a captured step) and REFILLED IN PLACE when the version counter of
    the storage owner moved (load_state_dict, the in-place refresh of another cached copy), so that HIP graphs that captured the buffer's
    address stay valid.  An entry serves the owner OBJECT it was made for: another tensor that lands on the same address gets a new buffer.
    A weight whose owner `cacheable` turns down (a `.contiguous()` copy of a misaligned window, a padded temporary) is derived afresh at
    every use into a buffer of its own: replacing a cached buffer would free memory that a captured graph still reads.  `refresh()`
    refills every live entry (functional.refresh_caches).
    CONTRACT: validity is keyed on torch's version counter of the owner.  A write that bypasses it -- `p.data.copy_()`, `p.data.mul_()`, a
    custom kernel writing a frozen weight -- leaves the buffer stale without any error: call functional.refresh_caches(model) after such
    a write (README "Changing frozen weights").  train.TrainStep calls it at construction.
    `trainable`, TRAINABLE weights inside a step driver (functional.managed_weights sets `managed`): persistent too, and ALL refilled by
    one `refresh_batch` call at the start of every step, i.e. after whatever changed the weights (the flat AdamW kernel writes them
    without touching version counters).  Outside a driver a trainable weight is derived afresh at every use.
    make(w, tag) -> derived; refill(w, derived, tag); cacheable(owner) -> bool; refresh_batch([(view, derived, tag)]); what: for messages."""

    LIMIT = 1024                       # dead entries are swept when the frozen table grows past this
    managed = False
    trainable_anchor = staticmethod(lambda w: w._base if w._base is not None else w)

    def __init__(self, what, make, refill, cacheable=any_owner, refresh_batch=None):
        self.what, self.make, self.refill, self.cacheable, self.refresh_batch = what, make, refill, cacheable, refresh_batch
        self.entries = {}
        self.trainable = {}

    def get(self, w):
        owner = w._base if w._base is not None else w
        if not self.cacheable(owner):
            return self.make(w, None)
        key = (w.data_ptr(), tuple(w.shape), tuple(w.stride()))
        e = self.entries.get(key)
        if e is None or e.anchor() is not owner:
            if len(self.entries) > self.LIMIT:
                self.entries = {k: v for k, v in self.entries.items() if v.anchor() is not None}
            e = self.entries[key] = Entry(owner, owner._version, self.make(w, None), key[1:] + (w.storage_offset(),))
        elif e.version != owner._version:
            if w.is_cuda and torch.cuda.is_current_stream_capturing():
                # a refill here would be baked into the graph as a launch of its own: refuse loudly instead of multiplying by the old weight
                raise RuntimeError("upp_hip: a frozen weight changed after its %s was made and the stream is capturing; call "
                                   "upp_hip.functional.refresh_caches(model) after changing weights and before capturing a step" % self.what)
            self.refill(w, e.derived, None)
            e.version = owner._version
        return e.derived

    def refresh(self):
        for e in self.entries.values():
            if e.anchor() is not None:
                self.refill(e.view(), e.derived, None)
                e.version = e.anchor()._version

    def get_trainable(self, w, transposed=False, tag=None):
        tag = bool(transposed) if tag is None else tag
        owner = w._base if w._base is not None else w
        if not self.cacheable(owner):                # a computed weight (padded, concatenated ...): derived where it is used
            return self.make(w.detach(), tag)
        key = (w.data_ptr(), tuple(w.shape), tuple(w.stride()), tag)
        e = self.trainable.get(key)
        if e is None or e.owner() is not owner:
            e = self.trainable[key] = Entry(self.trainable_anchor(w), None, self.make(w.detach(), tag), key[1:3] + (w.storage_offset(),), tag)
        return e.derived

    def refresh_trainable(self, owners=None):
        """owners: a set of id()s of parameters -- only their buffers (an evaluation graph refreshes the weights of ITS model)."""
        self.trainable = {k: e for k, e in self.trainable.items() if e.anchor() is not None}
        jobs = [(e.view(), e.derived, e.tag) for e in self.trainable.values() if owners is None or id(e.owner()) in owners]
        if jobs:
            self.refresh_batch(jobs)


@contextlib.contextmanager
def managed(caches, owners=None):
    """Scope of a step driver: sets `managed` on the caches, refreshes their trainable buffers (in the order given), restores the flags."""
    was = [c.managed for c in caches]
    for c in caches:
        c.managed = True
    try:
        for c in caches:
            c.refresh_trainable(owners)
        yield
    finally:
        for c, flag in zip(caches, was):
            c.managed = flag
