"""Per-batch memos: what the framework remembers about a batch on the batch's own tensors (CSR topology, species groups, row
pointers, the flat species index, knot bins built ahead of the step, stream aliases, the per-forward stack caches).

Storage: one attribute on the tensor, ``t._e3k_memo`` = {slot: (version, key, value)}, so a memo lives exactly as long as its
tensor; ``clone()`` and ``view()`` results do not carry it.

Validity, the same for every slot: the tensor has not been written to since (``t._version`` is the one at ``remember``; ``copy_``
and ``torch._foreach_copy_`` into the tensor bump it) and ``key`` -- whatever else the value depends on: ``num_nodes``, ``n_keys``,
a device, ``r_max`` -- equals the stored key.

A value must not hold a strong reference to its own tensor, a view of it included: a view keeps a C++ reference to its base, and
tensor -> attribute -> view -> tensor is a cycle through the C++ reference counts that nothing ever collects.  Remember a copy, or
a ``weakref`` to the view (the stream alias does).

Recording: a memo that hits while a stream is capturing keeps its kernels OUT of the HIP graph.  That is intended for a batch
prepared ahead by ``prepare_data`` (``PipelinedBucketedStep``: the preparation is a graph of its own) and for one resident batch
(``bench.py --graph``, a bare ``CapturedStep``).  A step whose input contents change between replays must ``forget`` its static
batch before it records (``BucketedStep`` does): the replay would otherwise walk the warm-up batch's topology.
"""
import torch

_ATTR = "_e3k_memo"


def recall(t, slot, *key):
    """The value remembered on ``t`` under ``slot`` (any hashable) for this ``key`` and the tensor's present contents, or None."""
    hit = getattr(t, _ATTR, {}).get(slot)
    return hit[2] if hit is not None and hit[0] == t._version and hit[1] == key else None


def remember(t, slot, value, *key):
    memos = getattr(t, _ATTR, None)
    if memos is None:
        memos = {}
        setattr(t, _ATTR, memos)
    memos[slot] = (t._version, key, value)
    return value


def forget(batch) -> None:
    """Drops every memo held by the batch's tensors (the marks that say what a tensor IS, ``_e3k_key`` and the like, stay)."""
    for k in batch.keys():
        v = batch[k]
        if torch.is_tensor(v) and hasattr(v, _ATTR):
            delattr(v, _ATTR)
