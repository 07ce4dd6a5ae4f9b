"""upp_hip._derived.DerivedWeights, the one cache behind functional.TRANSPOSED (W^T copies) and ops.PLANES (bf16 plane images), driven on
the CPU with pure-torch callables (the derived buffer is a transpose) under both owner policies.  The refusal of a stale buffer under
capture needs a capturing stream: tests/test_gpu_linear_sb.py keeps it."""
import gc

import pytest
import torch

from upp_hip import _derived


def _cache(policy, batches=None):
    made = []

    def make(w, tag):
        made.append(tag)
        return w.detach().t().contiguous()

    def refill(w, wt, tag):
        wt.copy_(w.detach().t())

    def refresh_batch(jobs):
        batches.append(jobs)
        for w, wt, tag in jobs:
            refill(w, wt, tag)

    c = _derived.DerivedWeights("transpose", make, refill, policy, refresh_batch)
    c.made = made
    return c


def _weight(policy, *shape):
    """A tensor the policy lets the cache keep."""
    w = torch.randn(*shape)
    if policy is _derived.persistent_owner:
        w._upp_persistent = True
    return w


POLICIES = pytest.mark.parametrize("policy", [_derived.any_owner, _derived.persistent_owner], ids=["any", "persistent"])


@POLICIES
def test_one_entry_per_window_refreshed_in_place_and_bound_to_its_owner(policy):
    c = _cache(policy)
    big = _weight(policy, 3, 8)
    left, right = c.get(big[:, :4]), c.get(big[:, 4:])
    assert len(c.entries) == 2 and left is not right                       # two windows of one parameter: two entries
    assert c.get(big[:, 4:]) is right and len(c.made) == 2                 # ... each served again, to a new view object too
    assert set(c.entries) == {(v.data_ptr(), tuple(v.shape), tuple(v.stride())) for v in (big[:, :4], big[:, 4:])}
    big.mul_(2.0)                                                          # the owner's version moves: the windows' too
    assert c.get(big[:, 4:]) is right and torch.equal(right, big[:, 4:].t()) and len(c.made) == 2      # refilled in place
    w = _weight(policy, 3, 4)
    t1 = c.get(w)
    other = _weight(policy, 3, 4)
    c.entries[(other.data_ptr(), tuple(other.shape), tuple(other.stride()))] = c.entries[(w.data_ptr(), tuple(w.shape), tuple(w.stride()))]
    t2 = c.get(other)                                                      # "another tensor landed on this address"
    assert t2 is not t1 and torch.equal(t2, other.t()) and torch.equal(t1, w.t())


def test_the_persistent_policy_never_stores_a_temporary():
    c = _cache(_derived.persistent_owner)
    tmp = torch.randn(3, 4)
    a, b = c.get(tmp), c.get(tmp)
    assert a is not b and torch.equal(a, b) and not c.entries              # derived afresh at each call, never stored
    assert c.get_trainable(tmp) is not c.get_trainable(tmp) and not c.trainable
    tmp._upp_persistent = True
    assert c.get(tmp) is c.get(tmp) and len(c.entries) == 1
    p = torch.nn.Parameter(torch.randn(3, 4))
    assert c.get(p) is c.get(p) and c.get(p[:, 1:]) is c.get(p[:, 1:]) and len(c.entries) == 3
    assert _cache(_derived.any_owner).get(torch.randn(3, 4)) is not None


@POLICIES
def test_refresh_rederives_even_when_the_version_did_not_move(policy):
    c = _cache(policy)
    w = _weight(policy, 3, 4)
    win = w[:, 2:]
    t, tw = c.get(w), c.get(win)
    w.data.copy_(torch.ones(3, 4))                                         # a write that bypasses the version counter
    assert c.get(w) is t and not torch.equal(t, w.t())                     # (the documented blind spot)
    c.refresh()
    assert c.get(w) is t and torch.equal(t, torch.ones(4, 3)) and torch.equal(tw, torch.ones(2, 3))
    with torch.no_grad():
        w.mul_(3.0)
    for e in c.entries.values():
        e.version = w._version                                             # pretend nobody noticed
    c.refresh()
    assert torch.equal(t, torch.full((4, 3), 3.0))


@POLICIES
def test_the_sweep_past_the_limit_keeps_every_live_entry(policy):
    c = _cache(policy)
    live = [_weight(policy, 2, 2) for _ in range(10)]
    kept = [c.get(w) for w in live]
    crowd = [_weight(policy, 2, 2) for _ in range(c.LIMIT + 6)]
    for w in crowd:
        c.get(w)                                                           # (sweeps from entry 1,026 on find nothing dead)
    assert c.LIMIT == 1024 and len(c.entries) == 10 + len(crowd)
    del crowd, w
    gc.collect()
    late = _weight(policy, 2, 2)
    c.get(late)                                                            # the table is past the limit: this insertion sweeps it
    assert len(c.entries) == 11 and all(e.anchor() is not None for e in c.entries.values())
    n = len(c.made)
    assert all(c.get(w) is t for w, t in zip(live, kept)) and len(c.made) == n          # every live entry survived, still served


def test_refresh_trainable_drops_the_dead_names_owners_and_launches_once():
    batches = []
    c = _cache(_derived.persistent_owner, batches)
    ps = [torch.nn.Parameter(torch.randn(3, 4)) for _ in range(4)]
    ts = [c.get_trainable(p) for p in ps]
    tw = c.get_trainable(ps[0][:, 2:])                                     # a window: anchored at its parameter
    tt = c.get_trainable(ps[1], transposed=True)
    assert c.get_trainable(ps[0]) is ts[0] and c.get_trainable(ps[1], transposed=True) is tt is not ts[1] and len(c.trainable) == 6
    with torch.no_grad():
        for p in ps:
            p.add_(1.0)
    del p
    assert not torch.equal(ts[0], ps[0].t())                               # persistent: stale until the step driver refreshes
    del ps[3]
    gc.collect()
    c.refresh_trainable()
    assert len(batches) == 1 and len(batches[0]) == 5 and len(c.trainable) == 5          # one call for the lot; the dead entry is gone
    assert sorted(tag for _, _, tag in batches[0]) == [False, False, False, False, True]
    assert all(torch.equal(t, p.t()) for t, p in zip(ts, ps)) and torch.equal(tw, ps[0][:, 2:].t())
    c.refresh_trainable({id(ps[0])})
    assert len(batches) == 2 and [tuple(w.shape) for w, _, _ in batches[1]] == [(3, 4), (3, 2)]      # only the named owner's entries
    c.refresh_trainable(set())
    assert len(batches) == 2                                               # nothing to refresh: no call


def test_the_managed_scope_sets_refreshes_restores_and_nests():
    order = []
    a, b = _cache(_derived.any_owner), _cache(_derived.any_owner)
    a.refresh_trainable = lambda owners=None: order.append(("a", owners, a.managed))
    b.refresh_trainable = lambda owners=None: order.append(("b", owners, b.managed))
    with _derived.managed([a, b], owners={1}):
        assert a.managed and b.managed and order == [("a", {1}, True), ("b", {1}, True)]
        with _derived.managed([b]):
            assert b.managed
        assert a.managed and b.managed                                     # the inner scope put back what it found: still set
    assert not a.managed and not b.managed
    b.managed = True                                                       # an outer driver already holds b
    with pytest.raises(ValueError):
        with _derived.managed([a, b]):
            assert a.managed and b.managed
            raise ValueError("inside")
    assert not a.managed and b.managed                                     # restored to the previous values after an exception too
    a.refresh_trainable = lambda owners=None: (_ for _ in ()).throw(RuntimeError("refresh"))
    with pytest.raises(RuntimeError):
        with _derived.managed([a]):
            pass
    assert not a.managed


def test_both_library_caches_are_instances_of_the_shared_class():
    from upp_hip import functional as HF, ops
    assert isinstance(HF.TRANSPOSED, _derived.DerivedWeights) and isinstance(ops.PLANES, _derived.DerivedWeights)
    was = HF.TRANSPOSED.managed, ops.PLANES.managed
    with HF.managed_weights(transposes=False):
        assert ops.PLANES.managed and HF.TRANSPOSED.managed == was[0]
    with HF.managed_weights():
        assert ops.PLANES.managed and HF.TRANSPOSED.managed
    assert (HF.TRANSPOSED.managed, ops.PLANES.managed) == was
