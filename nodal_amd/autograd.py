"""torch.autograd over the circuit solve: component values in, solutions out, gradients back through the adjoint.

    x = autograd.solve(circuit, values)                                   # [K+B]
    X = autograd.solve_sources(circuit, values, names, source_values)     # [M, K+B]
    W = autograd.transient(circuit, values, capacitors, dt, steps, ...)   # [steps+1, P]
    W = autograd.ac(circuit, values, capacitors, inductors, frequencies, ...)  # [F, P] complex
    x = autograd.operating_point(circuit, values, diodes, i_sat, n_vt, ...)    # [K+B]

`values` is a float64 CPU tensor [ncomp] in the order of `netlist.component_keys` (what `Circuit.values` holds),
`source_values` a float64 CPU tensor [M, len(names)] with the members' values of the swept A / E components
`names`.  Forward is `Circuit.set_values` + `solve()` / `solve_sources()` on the device; backward hands the incoming
cotangents to `Circuit.gradient` (nodal_gradient: one adjoint solve per member, the sum over the members formed on
the device) and is differentiable once.  The gradient for `values` is zero at the swept rows of solve_sources --
their table value is not used by any member -- and the swept values get theirs through `source_values`.
`transient` returns the probe waveforms of `Circuit.transient(..., record=True)`; its backward is
`Circuit.transient_gradient` (the time stepping run backwards) and hands gradients to `values`, the capacitances and
`source_values` [steps, len(names)]; at a swept row `values` gets what the DC start owes to the table value, zero when
the run starts from `initial`.
`ac` returns the probe phasors of `Circuit.ac`, complex128 [F, P]; its backward is one `Circuit.ac_gradient` call with the
incoming cotangent (torch's dL/dRe + j dL/dIm for a complex tensor is the convention of that call) and hands gradients to
`values`, the farads, the henries and the complex amplitudes.
`operating_point` returns the x of `Circuit.operating_point`, the nonlinear DC solution with diodes; its backward is one
`OperatingPoint.gradient` call (nodal_newton_gradient: one adjoint solve with the Newton matrix linearised at x) and
hands gradients to `values`, the diodes' `i_sat` and `n_vt` and `source_values` [len(names)]; at a named source's row
`values` gets zero.

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


class _Transient(torch.autograd.Function):
    @staticmethod
    def forward(ctx, circuit, values, farads, source_values, leads, dt, steps, names, probes, initial):
        held, caps = _values_of(values), _values_of(farads)
        names = list(names)
        swept = _values_of(source_values) if names else np.zeros((steps, 0))
        if swept.shape != (steps, len(names)):
            raise ValueError(f"source_values must have shape ({steps}, {len(names)}), not {tuple(swept.shape)}")
        if caps.shape != (len(leads),):
            raise ValueError(f"the farads must have shape ({len(leads)},), not {tuple(caps.shape)}")
        ctx.circuit, ctx.held, ctx.names = circuit, held, names
        ctx.call = dict(capacitors=[(name, float(f), a, b) for (name, a, b), f in zip(leads, caps)], dt=dt, steps=steps,
                        sources={name: swept[:, j] for j, name in enumerate(names)}, probes=list(probes),
                        initial=None if initial is None else np.array(initial, dtype=np.float64))
        tr = _Transient.run(ctx)
        return torch.from_numpy(np.array(tr.waveforms, dtype=np.float64))

    @staticmethod
    def run(ctx):
        circuit = ctx.circuit
        circuit.set_values(ctx.held)
        if ctx.call["initial"] is None:
            circuit.solve()
        tr = circuit.transient(record=True, **ctx.call)
        ctx.record = circuit._transient_record
        return tr

    @staticmethod
    @once_differentiable
    def backward(ctx, cotangent):
        circuit = ctx.circuit
        if ctx.record is None or circuit._transient_record is not ctx.record:
            _Transient.run(ctx)  # (the circuit has been used otherwise since the forward pass)
        grad = circuit.transient_gradient(_values_of(cotangent))
        from .sweep import resolve_sources
        values = np.array(grad.values, dtype=np.float64)
        rows, _ = resolve_sources(circuit.netlist, ctx.call["sources"])
        # (no step uses the table value of a swept source: it acts through the DC start alone, not at all with `initial`)
        values[rows] = grad.start_values[rows]
        swept = np.stack([grad.source_values[name] for name in ctx.names], axis=1) if ctx.names else None
        return (None, torch.from_numpy(values), torch.from_numpy(np.array(grad.capacitors, dtype=np.float64)),
                torch.from_numpy(np.ascontiguousarray(swept)) if ctx.names else None, None, None, None, None, None, None)


class _AC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, circuit, values, farads, henries, amplitudes, cap_leads, ind_leads, frequencies, names, probes):
        held, caps, inds = _values_of(values), _values_of(farads), _values_of(henries)
        names = list(names)
        if amplitudes.dtype != torch.complex128 or amplitudes.device.type != "cpu":
            raise TypeError("the amplitudes must be a complex128 CPU tensor")
        amps = np.array(amplitudes.detach().numpy(), dtype=np.complex128)
        if amps.shape != (len(names),):
            raise ValueError(f"the amplitudes must have shape ({len(names)},), not {tuple(amps.shape)}")
        if caps.shape != (len(cap_leads),) or inds.shape != (len(ind_leads),):
            raise ValueError("one value per capacitor and per inductor")
        ctx.circuit, ctx.held, ctx.names = circuit, held, names
        ctx.call = dict(frequencies=np.array(frequencies, dtype=np.float64),
                        capacitors=[(name, float(f), a, b) for (name, a, b), f in zip(cap_leads, caps)],
                        inductors=[(name, float(f), a, b) for (name, a, b), f in zip(ind_leads, inds)],
                        sources={name: complex(v) for name, v in zip(names, amps)} if names else None,
                        probes=list(probes))
        circuit.set_values(held)
        sweep = circuit.ac(**ctx.call)
        return torch.from_numpy(np.array(sweep.phasors, dtype=np.complex128))

    @staticmethod
    @once_differentiable
    def backward(ctx, cotangent):
        circuit = ctx.circuit
        _put_back(circuit, ctx.held)
        if cotangent.dtype != torch.complex128 or cotangent.device.type != "cpu":
            raise TypeError("nodal_amd.autograd.ac works on complex128 CPU phasors")
        grad = circuit.ac_gradient(cotangents=np.array(cotangent.detach().numpy(), dtype=np.complex128), **ctx.call)
        amps = np.array([grad.sources[name] for name in ctx.names], dtype=np.complex128).reshape(len(ctx.names))
        return (None, torch.from_numpy(np.array(grad.values, dtype=np.float64)),
                torch.from_numpy(np.array(grad.capacitors, dtype=np.float64)),
                torch.from_numpy(np.array(grad.inductors, dtype=np.float64)), torch.from_numpy(amps),
                None, None, None, None, None)


class _OperatingPoint(torch.autograd.Function):
    @staticmethod
    def forward(ctx, circuit, values, i_sat, n_vt, source_values, leads, names, options):
        held, sat, nvt = _values_of(values), _values_of(i_sat), _values_of(n_vt)
        names = list(names)
        swept = _values_of(source_values) if names else np.zeros(0)
        if swept.shape != (len(names),):
            raise ValueError(f"source_values must have shape ({len(names)},), not {tuple(swept.shape)}")
        if sat.shape != (len(leads),) or nvt.shape != (len(leads),):
            raise ValueError(f"i_sat and n_vt must have shape ({len(leads)},)")
        ctx.circuit, ctx.held, ctx.names = circuit, held, names
        ctx.call = dict(diodes=[(name, float(s), float(v), a, b) for (name, a, b), s, v in zip(leads, sat, nvt)],
                        sources={name: float(swept[j]) for j, name in enumerate(names)} if names else None,
                        **dict(options))
        circuit.set_values(held)
        ctx.op = circuit.operating_point(**ctx.call)
        return torch.from_numpy(np.array(ctx.op.x, dtype=np.float64))

    @staticmethod
    @once_differentiable
    def backward(ctx, cotangent):
        circuit = ctx.circuit
        _put_back(circuit, ctx.held)
        grad = ctx.op.gradient(_values_of(cotangent))
        values = np.array(grad.values, dtype=np.float64)
        if ctx.names:
            values[np.asarray(ctx.op.source_rows)] = 0.0  # (the run does not use the table value of a named source)
        swept = np.array([grad.source_values[name] for name in ctx.names], dtype=np.float64).reshape(len(ctx.names))
        return (None, torch.from_numpy(values), torch.from_numpy(np.array(grad.i_sat, dtype=np.float64)),
                torch.from_numpy(np.array(grad.n_vt, dtype=np.float64)), torch.from_numpy(swept) if ctx.names else None,
                None, None, None)


def solve(circuit, values):
    """The solution [K+B] of `circuit` with the component values `values` [ncomp], differentiable in `values`."""
    return _Solve.apply(circuit, values)


def solve_sources(circuit, values, names, source_values):
    """The solutions [M, K+B] of `circuit` with the component values `values` [ncomp] and, member by member, the
    values `source_values` [M, len(names)] of the independent sources `names`; differentiable in both."""
    return _SolveSources.apply(circuit, values, names, source_values)


def transient(circuit, values, capacitors, dt, steps, source_names=(), source_values=None, probes=(), initial=None):
    """The probe waveforms [steps+1, P] of `Circuit.transient` (backward Euler) with the component values `values`
    [ncomp], the capacitors `capacitors` -- (name, farads, node_a, node_b) with each farads a float64 CPU scalar
    tensor, e.g. an element of one [C] tensor -- and, step by step, the values `source_values` [steps,
    len(source_names)] of the independent sources `source_names`; differentiable in values, farads and source values.
    initial=None starts from the DC operating point of `values`, whose dependence on them is part of the gradient."""
    capacitors = list(capacitors)
    farads = torch.stack([torch.as_tensor(cap[1], dtype=torch.float64) for cap in capacitors]) if capacitors else \
        torch.zeros(0, dtype=torch.float64)
    leads = [(cap[0], cap[2], cap[3]) for cap in capacitors]
    if source_values is None:
        source_values = torch.zeros((steps, 0), dtype=torch.float64)
    return _Transient.apply(circuit, values, farads, source_values, leads, dt, steps, tuple(source_names), tuple(probes),
                            initial)


def ac(circuit, values, capacitors, inductors, frequencies, source_names=(), amplitudes=None, probes=()):
    """The probe phasors complex128 [F, P] of `Circuit.ac` at `frequencies` (Hz) with the component values `values`
    [ncomp], the capacitors and inductors -- (name, farads or henries, node_a, node_b) with each value a float64 CPU
    scalar tensor, e.g. an element of one tensor -- and the complex amplitudes `amplitudes` complex128 [len(source_names)]
    of the independent sources `source_names`, every other one off; differentiable in values, farads, henries and
    amplitudes.  The table value of an A / E row is never read: its gradient is exactly zero."""
    def split(elements):
        elements = list(elements)
        held = torch.stack([torch.as_tensor(e[1], dtype=torch.float64) for e in elements]) if elements else \
            torch.zeros(0, dtype=torch.float64)
        return held, [(e[0], e[2], e[3]) for e in elements]
    farads, cap_leads = split(capacitors)
    henries, ind_leads = split(inductors)
    if amplitudes is None:
        amplitudes = torch.zeros(0, dtype=torch.complex128)
    return _AC.apply(circuit, values, farads, henries, amplitudes, cap_leads, ind_leads, tuple(frequencies), tuple(source_names),
                     tuple(probes))


def operating_point(circuit, values, diodes, i_sat, n_vt, source_names=(), source_values=None, **newton_options):
    """The operating point x [K+B] of `Circuit.operating_point` with the component values `values` [ncomp], the diodes
    `diodes` -- (name, anode, cathode), plain -- with the parameters `i_sat` and `n_vt` [D] and the values
    `source_values` [len(source_names)] of the independent sources `source_names`; differentiable in values, i_sat, n_vt
    and source values.  `newton_options` go to Circuit.operating_point (initial, max_iter, reltol, vntol, abstol, gmin).
    The gradient is that of the exact operating point the iteration approximates: tighten the tolerances where the
    fourth digit of x matters."""
    leads = [(d[0], d[1], d[2]) for d in diodes]
    if source_values is None:
        source_values = torch.zeros(0, dtype=torch.float64)
    return _OperatingPoint.apply(circuit, values, i_sat, n_vt, source_values, leads, tuple(source_names),
                                 tuple(sorted(newton_options.items())))
