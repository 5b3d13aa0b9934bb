"""One MessagePassing layer (FactorizedConvolution + Gate) as ONE autograd node.

The arithmetic is the kernels' (``csrc/``); between them sits the host.  Composed from one ``autograd.Function`` per
kernel, a convolution layer costs ~12 Function applies forward and ~12 graph nodes backward, each with its own
argument checks, context bookkeeping, stream switches and engine hand-offs: 0.45 + 0.5 ms of Python per layer and
step -- at 256 molecules the host enqueue time (6.0 ms per step) had caught up with the GPU time (7.1 ms), so faster
kernels stopped paying.  Here the launches of a layer's forward (and of its backward) are issued by one C call of the
native layer executor (``csrc/e3k_layer.hip``, through ``conv_native.NativeConvBlockFn``), on the same three streams
(radial MLP | self-connection | node features -> tensor product) plus the weight-gradient stream, with explicit events
instead of autograd's per-node stream hand-offs.  This module holds the layer's static plan, the stream helpers and the
entry point; ``MessagePassing._block_plan`` hands out a plan only for layers the executor takes.

What it replaces (reference, per layer): ``FactorizedConvolution.forward`` + ``Gate``
(``e3_layers/nn/message_passing.py:91-124, 249``).  The composed path stays -- it is the readable definition, it serves
double backward (force training), un-keyed node attributes, the 'norm' nonlinearity -- and ``E3K_CONV_BLOCK=0``
forces it; ``tests/test_gpu_model.py::test_conv_block_equals_composed_layers`` pins the two against each other.
"""
from __future__ import annotations

from typing import Sequence

import torch

from .tuning import knob as _knob

from . import conv_native, ops

ENABLED = _knob("E3K_CONV_BLOCK")
LOOK_AHEAD = _knob("E3K_BLOCK_LOOK_AHEAD")     # the next layer's radial branch issued one layer early
AHEAD_STATS = [0]      # look-ahead results consumed (tests)


class ConvBlockPlan:
    """Static description of one layer (specs own their cached launch descriptors)."""

    def __init__(self, *, in_blocks, lin1_spec, mlp_alphas, mlp_act, mlp_cst, mlp_k0, last_spec, tp_plan, post_spec, scale,
                 sc_spec, sc_m_off, sc_ld_m, gate_spec, addend: bool = False):
        self.in_blocks, self.lin1_spec = in_blocks, lin1_spec
        # addend: the self-connection is NOT part of the block (general, un-keyed node attributes: the outer-product form of
        # ops.fctp); its output [N, d_conv] (cf) is handed in, the trailing Linear accumulates on top of it, and the backward
        # hands the gradient of the convolution output back for it (travels in the ``m_pre`` slot)
        self.addend = bool(addend)
        self.mlp_alphas, self.mlp_act, self.mlp_cst, self.last_spec = tuple(mlp_alphas), mlp_act, float(mlp_cst), last_spec
        self.mlp_k0 = int(mlp_k0)
        self.tp_plan, self.post_spec, self.scale = tp_plan, post_spec, float(scale)
        self.sc_spec, self.sc_m_off, self.sc_ld_m = sc_spec, tuple(sc_m_off) if sc_m_off is not None else None, sc_ld_m
        self.gate_spec = gate_spec
        self.prefetched = None     # radial branch of THIS layer issued by the previous layer's forward (look-ahead)
        self.guard_key = None      # the radial MLP's last-layer Parameter: key of its knot-table guard (radial_table.guard)

    def replace(self, **fields) -> "ConvBlockPlan":
        """A NEW plan with the named constructor fields substituted (``conv_native.NativeLayer.narrow``: the same layer with pruned
        specs).  Built through the constructor: per-object state and caches (``prefetched``, the executor's layer object, whatever
        is cached on a plan later) start empty."""
        args = dict(in_blocks=self.in_blocks, lin1_spec=self.lin1_spec, mlp_alphas=self.mlp_alphas, mlp_act=self.mlp_act,
                    mlp_cst=self.mlp_cst, mlp_k0=self.mlp_k0, last_spec=self.last_spec, tp_plan=self.tp_plan, post_spec=self.post_spec,
                    scale=self.scale, sc_spec=self.sc_spec, sc_m_off=self.sc_m_off, sc_ld_m=self.sc_ld_m, gate_spec=self.gate_spec,
                    addend=self.addend)
        unknown = set(fields) - set(args)
        if unknown:
            raise TypeError(f"ConvBlockPlan.replace: no such field {sorted(unknown)}")
        args.update(fields)
        new = ConvBlockPlan(**args)
        new.guard_key = self.guard_key
        return new


class _on:
    """``with _on(stream, main)``: launches go to ``stream`` (no-op when it is ``main``)."""

    __slots__ = ("st", "main")

    def __init__(self, st, main):
        self.st, self.main = st, main

    def __enter__(self):
        if self.st is not self.main:
            torch.cuda.set_stream(self.st)

    def __exit__(self, *exc):
        if self.st is not self.main:
            torch.cuda.set_stream(self.main)
        return False


def _wait(consumer, producer):
    if consumer is not producer:
        consumer.wait_stream(producer)


def _grad_buffer(weight, need: bool):
    """(buffer to accumulate into, tensor to return to autograd) for one parameter."""
    if not need:
        return None, None
    sink = ops._sink_for(weight)
    if sink is not None:
        return sink, None
    buf = torch.zeros_like(weight)
    return buf.view(-1), buf


def conv_block(x, node_attrs, edge_radial, sh, plan: ConvBlockPlan, topo, groups, in_cf: bool, out_cf: bool, fork: bool,
               w_lin1, w_post, w_sc, w_last, w_hidden: Sequence[torch.Tensor], table=None, nxt=None, pre=None, m_pre=None):
    if m_pre is not None:    # the per-key self-connection weights of this layer come from conv_native.KwStackFn
        node_attrs = w_sc = None
    if pre is not None:      # stack mode: the radial MLP's rows of this layer come from conv_native.RadialStackFn
        return conv_native.NativeConvBlockFn.apply(x, node_attrs, None, sh, plan, topo, groups, in_cf, out_cf, fork, table, nxt,
                                                   pre, m_pre, w_lin1, w_post, w_sc, None)
    out = conv_native.NativeConvBlockFn.apply(x, node_attrs, edge_radial, sh, plan, topo, groups, in_cf, out_cf, fork, table,
                                              nxt, None, m_pre, w_lin1, w_post, w_sc, w_last, *w_hidden)
    return out[0] if isinstance(out, tuple) else out      # (addend form: the dirtied addend rides along as a second output)
