"""Output heads: ``GradientOutput`` (forces / scores by autograd through the HIP kernels) and
``Pooling`` — interfaces of ``e3_layers/nn/output.py:19-53,56-74``.  ``Pairwise`` and
``TensorProductContraction`` (legacy Hamiltonian head) are out of scope.
"""
from __future__ import annotations

import torch

from ..backend import memo, ops
from ..o3 import Irreps
from ..utils.utils import _is_mapping, build
from .sequential import Module


class GradientOutput(Module):
    """``gradients = sign d y / d x`` by autograd through the HIP kernels.

    ``virial`` / ``stress``: output keys (None: not emitted; plain attributes, ``enable_virial`` sets them on a built tree).  With ``x``
    the positions, the backward of the edge vectors also files, per graph of the batch as given (the ghost graph of a padded one
    included) and in the row-vector convention of ``cell`` (``x -> x (I + eps)``, ``cell -> cell (I + eps)``),

        virial[g, 3 a + b] = -dE_g / d eps_ab = -sum_{e in g} v_e[a] (dE / dv_e)[b]        (nequip's sign; open cluster: sum_n x_n (x) F_n)
        stress = -virial / |det cell|                                                       (ASE's sign: (1 / V) dE / d eps; det = 0: zero)

    both ``[G, 9]`` fp32 with attrs ``("graph", "3x1o")``, the layout of ``cell``; all nine components, nothing symmetrised.  One launch
    more (``e3k_virial_edges``), from the per-edge gradients the forces are made of.  Refused: ``stress`` without a ``cell`` in the
    batch (``ValueError``); training mode, where the gradient's own graph is kept (``NotImplementedError``: stress training is not
    served); edge vectors the caller supplied, so that no edge-vector function runs (``NotImplementedError``)."""

    def __init__(self, func, x, y, gradients, sign: float = 1.0, virial: str = None, stress: str = None, **kwargs):
        super().__init__()
        sign = float(sign)
        assert sign in (1.0, -1.0)
        self.sign = sign
        self.virial, self.stress = virial, stress
        self.init_irreps(x=x, y=y, gradients=gradients, output_keys=["gradients"])
        assert Irreps(self.irreps_in["y"]).lmax == 0
        if _is_mapping(func):
            func = build(func, **kwargs)
        self.func = func

    def prepare_data(self, batch) -> dict:
        """``SequentialGraphNetwork.prepare_data`` of the wrapped network, minus everything that reads ``x``: the forward
        differentiates w.r.t. it, so edge vectors, lengths and spherical harmonics belong to the autograd graph of the step (what is
        left: topology, one-hot species, key groups)."""
        inner = getattr(self.func, "prepare_data", None)
        if inner is None:
            return {}
        x_key = next((g for g, loc in self.input_key_mapping.items() if loc == "x"), "x")
        return inner(batch, exclude=(x_key,))

    def _virial_request(self, data):
        """None when neither key is set; else the refusals that need no kernel, and the batch's graph counts."""
        if self.virial is None and self.stress is None:
            return None
        if self.training:
            raise NotImplementedError("GradientOutput: virial / stress in training mode is not served (the gradient's own graph is "
                                      "kept there, and the virial's second backward -- training on stress -- is not formed): call "
                                      "model.eval()")
        if self.stress is not None and "cell" not in data:
            raise ValueError(f"GradientOutput: the stress '{self.stress}' is the virial over the cell's volume, and the batch has no "
                             "'cell' (an open batch serves the virial only)")
        if "edge_vector" in data:      # (no edge-vector function would run: the sink below would never be written)
            raise NotImplementedError("GradientOutput: virial / stress with edge vectors the caller supplies ('edge_vector' in the batch) "
                                      "is not served: the virial is filed by the backward of the model's own edge-vector function")
        if "_n_nodes" not in data:
            raise ValueError("GradientOutput: the virial is summed per graph and needs the batch's '_n_nodes'")
        return data["_n_nodes"]

    def _emit_virial(self, data, output, buffer) -> None:
        if self.virial is not None:
            output.attrs[self.virial] = ("graph", "3x1o")
            output[self.virial] = buffer
        if self.stress is not None:
            c = data["cell"].reshape(-1, 9).to(buffer.dtype)
            if c.shape[0] != buffer.shape[0]:
                raise ValueError(f"GradientOutput: {c.shape[0]} cells for {buffer.shape[0]} graphs")
            # det = a . (b x c) of the rows; eight small launches in all (each is one more node of a captured graph)
            det = (c[:, 0:3] * torch.linalg.cross(c[:, 3:6], c[:, 6:9], dim=1)).sum(1, keepdim=True)
            minus_volume = det.abs().neg()
            output.attrs[self.stress] = ("graph", "3x1o")
            output[self.stress] = torch.where(minus_volume < 0, buffer / minus_volume, 0.0)      # (the ghost graph: det = 0)

    def forward(self, data):
        counts = self._virial_request(data)
        wrt = self.inputKeyMap(data)["x"]
        old = wrt.requires_grad
        wrt.requires_grad_(True)
        #  edge vectors the CALLER supplied and that require grad hang on some other leaf (a cell, a strain): the force
        # block's second pass hands back parameter gradients only, so the force-loss share of that leaf's gradient would be
        # missing -- such a call takes the composed path too
        pre = data.get("edge_vector") if "edge_vector" in data else None
        foreign = pre is not None and bool(pre.requires_grad)
        if (old and self.training) or foreign:
            # the caller differentiates w.r.t. ``x`` itself (it required grad before this call) and the graph of the gradient is
            # kept: d loss / d x of a loss on the gradients needs third derivatives of the layers -- the force block
            # (backend/conv_force.py) does not form them, the composed per-kernel path does
            from ..backend import conv_force

            with conv_force.declined():
                output = self.func(data)
        else:
            output = self.func(data)
        # only d y / d x is asked for: the backward functions skip every Parameter gradient of this pass
        if counts is None:
            with ops.inputs_only_backward():
                (grad,) = torch.autograd.grad(self.inputKeyMap(output)["y"].sum(), wrt, create_graph=self.training)
        else:
            # ... and the backward of the edge vectors files the virial of every graph of the batch as given (ops.virial_sink)
            buffer = torch.empty(counts.numel(), 9, device=wrt.device, dtype=torch.float32)
            with ops.virial_sink(buffer, Pooling._row_pointers(counts, wrt.device)) as sink, ops.inputs_only_backward():
                (grad,) = torch.autograd.grad(self.inputKeyMap(output)["y"].sum(), wrt, create_graph=False)
            if sink.written != 1:
                wrt.requires_grad_(old)
                raise NotImplementedError(
                    "GradientOutput: the virial is filed by the backward of the edge-vector function, which ran "
                    f"{sink.written} times: edge vectors the caller supplies ('edge_vector' in the batch) are not served")
            self._emit_virial(data, output, buffer)
        wrt.requires_grad_(old)
        is_per = self.inputKeyMap(data.attrs)["x"][0]
        output.attrs.update(self.outputKeyMap({"gradients": (is_per, self.irreps_out["gradients"])}))
        output.update(self.outputKeyMap({"gradients": self.sign * grad}))
        return output


def enable_virial(model, virial="virial", stress="stress"):
    """Sets the ``virial`` / ``stress`` output keys (None: off) on every ``GradientOutput`` of a built tree -- a model built from an
    unchanged config or loaded from a checkpoint -- and returns the model.  A tree without one is refused."""
    heads = [m for m in model.modules() if isinstance(m, GradientOutput)]
    if not heads:
        raise ValueError("enable_virial: the model has no GradientOutput (the virial is filed by the force backward)")
    for m in heads:
        m.virial, m.stress = virial, stress
    return model


class Pooling(Module):
    """node -> graph reduction over the (sorted) node segments."""

    def __init__(self, irreps_in, irreps_out, reduce):
        super().__init__()
        self.init_irreps(input=irreps_in, output=irreps_out, output_keys=["output"])
        assert reduce in ("sum", "mean")
        self.reduce = reduce

    @staticmethod
    def _row_pointers(counts, device):
        """int32 [G + 1] row pointers of the per-graph node counts; memoised on the counts tensor (``prepare_batch`` builds them
        ahead of the step: they are batch data)."""
        hit = memo.recall(counts, "ptr", device)
        if hit is not None:
            return hit
        n = counts.view(-1).to(device)
        if n.is_cuda and n.dtype == torch.int64 and n.is_contiguous():
            from ..backend.diffusion_ops import graph_row_pointers

            ptr = graph_row_pointers(n)
        else:
            ptr = torch.empty(n.numel() + 1, dtype=torch.int32, device=device)
            ptr[0] = 0
            ptr[1:] = torch.cumsum(n, 0).to(torch.int32)
        return memo.remember(counts, "ptr", ptr, device)

    def prepare_batch(self, network, data, avail) -> None:
        """``SequentialGraphNetwork.prepare_data`` hook: the segment pointers depend on ``_n_nodes`` alone."""
        if "_n_nodes" in avail and "_n_nodes" in data and data["_n_nodes"].is_cuda:
            self._row_pointers(data["_n_nodes"], data["_n_nodes"].device)

    def forward(self, data, attrs):
        x = data["input"]
        ptr = self._row_pointers(data["_n_nodes"], x.device)
        out = ops.segment_sum(x, ptr, data["_node_segment"].to(x.device), self.reduce == "mean")
        return {"output": out}, {"output": ("graph", self.irreps_out["output"])}
