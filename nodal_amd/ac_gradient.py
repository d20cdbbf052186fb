"""Gradients through frequency: the derivative of a loss of the AC phasors with respect to every component value, every
capacitance and inductance and every driven amplitude.

Someone who fits a network to a measured frequency response, tunes a decoupling network's resonance or moves a filter's
corner gets the response from `Circuit.ac`; its derivative by central differences costs two sweeps per component.  With
A(w) = G + j B(w) the matrix of `Circuit.ac`, A x = s the forward system and W[f][p] = x_f(a_p) - x_f(b_p) the probe
phasors, a real loss L has the cotangent g = dL/dRe W + j dL/dIm W (what torch hands back for a complex tensor), and ONE
adjoint solve per frequency, A(w)^T y = sum_p conj(g_p) (e(a_p) - e(b_p)) -- the plain transpose, nothing else is
conjugated -- gives dL = sum_f Re(y^T (ds - dA x)) for every parameter at once.  `Circuit.ac_gradient` hands the whole sweep
to `nodal_ac_gradient` (csrc/ac_gradient.hip): on a symmetric G the forward and the adjoint right-hand side go through
one numeric factorisation per frequency, and the per-row formulas are evaluated on the device, summed over the
frequencies there.

`check_ac_gradient_arguments` needs no device, and `ACGradient` is a plain container that can be built from arrays.
"""

import numpy as np


def check_ac_gradient_arguments(cotangents, nfreq, nprobes):
    """The cotangents of Circuit.ac_gradient as complex128 [nfreq, nprobes].  TypeError unless they are complex (a
    real array would silently drop dL/dIm), ValueError for another shape and for entries that are not finite."""
    cot = np.asarray(cotangents)
    if not np.iscomplexobj(cot):
        raise TypeError("cotangents must be complex: dL/dRe W + j dL/dIm W of the probe phasors")
    cot = np.ascontiguousarray(cot, dtype=np.complex128)
    want = (int(nfreq), int(nprobes))
    if cot.shape != want:
        raise ValueError(f"cotangents must have shape {want}, not {cot.shape}")
    if not (np.isfinite(cot.real).all() and np.isfinite(cot.imag).all()):
        raise ValueError("cotangents must be finite")
    return cot


class ACGradient:
    """Result of Circuit.ac_gradient, for a real loss L of the probe phasors.

    values [ncomp]: dL / d value of table row i, in the order of `netlist.component_keys`, summed over the frequencies;
    exactly 0.0 at A / E rows, whose table value the small-signal excitation never reads.  capacitors [C] and inductors
    [L]: dL/dC and dL/dL with respect to the farads and henries as passed, in the order they were passed, and
    capacitors_by_name / inductors_by_name the same by name.  sources: name -> complex, dL/dRe alpha + j dL/dIm alpha
    of the driven amplitude, summed over the frequencies and over the rows that carry the name; source_terms complex128
    [F, R], the term of every frequency and driven row, and source_rows [R] those rows.  phasors complex128 [F, P]:
    the forward phasors, as Circuit.ac gives them.  info [F]: 0 solved, > 0 singular at that frequency (sparse path: NaN
    in its rows and in all of values, capacitors, inductors and sources); scaled_residual [F, 2] of the forward and the
    adjoint system, computed on the device; adjoints complex128 [F, K+B] or None; work int64 [3]: numeric
    factorisations, block applications of the sparse factors, columns redone alone; timings: nodal_last_timings of the
    call, as after Circuit.ac."""

    def __init__(self, values, capacitors, inductors, sources, source_terms, phasors, info, scaled_residual,
                 capacitor_names=(), inductor_names=(), source_rows=None, adjoints=None, work=None, timings=None):
        self.values = values
        self.capacitors = capacitors
        self.inductors = inductors
        self.capacitor_names = list(capacitor_names)
        self.inductor_names = list(inductor_names)
        if len(self.capacitor_names) != len(capacitors) or len(self.inductor_names) != len(inductors):
            raise ValueError("one name per capacitor and per inductor")
        self.capacitors_by_name = {name: float(v) for name, v in zip(self.capacitor_names, capacitors)}
        self.inductors_by_name = {name: float(v) for name, v in zip(self.inductor_names, inductors)}
        self.sources = dict(sources)
        self.source_terms = source_terms
        self.source_rows = source_rows
        self.phasors = phasors
        self.info = info
        self.scaled_residual = scaled_residual
        self.adjoints = adjoints
        self.work = work
        self.timings = timings

    def __len__(self):
        return len(self.info)


def sources_by_name(keys, rows, source_terms):
    """name -> the sum of source_terms [F, R] over the frequencies and over the driven rows `rows` that carry the name
    (`keys`: netlist.component_keys), in row order"""
    out = {}
    for j, row in enumerate(np.asarray(rows).tolist()):
        name = keys[row]
        out[name] = out.get(name, 0j) + complex(source_terms[:, j].sum())
    return out
