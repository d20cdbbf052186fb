"""torch.autograd over the circuit solve: component values in, solutions out, gradients back through the adjoint.

    x = autograd.solve(circuit, values)                                   # [K+B]
    X = autograd.solve_sources(circuit, values, names, source_values)     # [M, K+B]

`values` is a float64 CPU tensor [ncomp] in the order of `netlist.component_keys` (what `Circuit.values` holds),
`source_values` a float64 CPU tensor [M, len(names)] with the members' values of the swept A / E components
`names`.  Forward is `Circuit.set_values` + `solve()` / `solve_sources()` on the device; backward hands the incoming
cotangents to `Circuit.gradient` (nodal_gradient: one adjoint solve per member, the sum over the members formed on
the device) and is differentiable once.  The gradient for `values` is zero at the swept rows of solve_sources --
their table value is not used by any member -- and the swept values get theirs through `source_values`.

This module imports torch; `import nodal_amd` does not import it.
"""

import numpy as np
import torch
from torch.autograd.function import once_differentiable


def _values_of(tensor):
    if tensor.dtype != torch.float64 or tensor.device.type != "cpu":
        raise TypeError("nodal_amd.autograd works on float64 CPU tensors")
    return np.array(tensor.detach().numpy(), dtype=np.float64)


def _put_back(circuit, values):
    """the saved values, if the circuit has been given others since the forward pass"""
    if not np.array_equal(np.asarray(circuit.values), values):
        circuit.set_values(values)


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, circuit, values):
        held = _values_of(values)
        circuit.set_values(held)
        x = np.array(circuit.solve().result, dtype=np.float64)
        ctx.circuit, ctx.held, ctx.x = circuit, held, x
        return torch.from_numpy(x.copy())

    @staticmethod
    @once_differentiable
    def backward(ctx, cotangent):
        circuit = ctx.circuit
        _put_back(circuit, ctx.held)
        grad = circuit.gradient(_values_of(cotangent), solutions=ctx.x)
        return None, torch.from_numpy(np.array(grad.values, dtype=np.float64))


class _SolveSources(torch.autograd.Function):
    @staticmethod
    def forward(ctx, circuit, values, names, source_values):
        held = _values_of(values)
        swept = _values_of(source_values)
        names = list(names)
        if swept.ndim != 2 or swept.shape[1] != len(names):
            raise ValueError(f"source_values must have shape (M, {len(names)}), not {tuple(swept.shape)}")
        circuit.set_values(held)
        sources = {name: swept[:, j] for j, name in enumerate(names)}
        x = np.array(circuit.solve_sources(sources).result, dtype=np.float64)
        ctx.circuit, ctx.held, ctx.sources, ctx.names, ctx.x = circuit, held, sources, names, x
        return torch.from_numpy(x.copy())

    @staticmethod
    @once_differentiable
    def backward(ctx, cotangent):
        from .sweep import resolve_sources
        circuit = ctx.circuit
        _put_back(circuit, ctx.held)
        grad = circuit.gradient(_values_of(cotangent), sources=ctx.sources, solutions=ctx.x)
        values = np.array(grad.values, dtype=np.float64)
        rows, _ = resolve_sources(circuit.netlist, ctx.sources)
        values[rows] = 0.0  # (no member uses the table value of a swept source)
        swept = np.stack([grad.source_values[name] for name in ctx.names], axis=1) if ctx.names else \
            np.zeros((len(ctx.x), 0))
        return None, torch.from_numpy(values), None, torch.from_numpy(np.ascontiguousarray(swept))


def solve(circuit, values):
    """The solution [K+B] of `circuit` with the component values `values` [ncomp], differentiable in `values`."""
    return _Solve.apply(circuit, values)


def solve_sources(circuit, values, names, source_values):
    """The solutions [M, K+B] of `circuit` with the component values `values` [ncomp] and, member by member, the
    values `source_values` [M, len(names)] of the independent sources `names`; differentiable in both."""
    return _SolveSources.apply(circuit, values, names, source_values)
