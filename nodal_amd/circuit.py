"""Circuit and Solution: the reference's Python seam over the HIP hot path.

Mirrors reference nodal/nodal.py:299-434 (`Circuit(netlist, sparse=False)`,
`.solve()`, `Solution`) with the same names, argument meaning and error
behaviour.  What the reference does with numpy/scipy on the host happens here
on an MI355X through libnodal_hip.so:

    Circuit.__init__ -> build_model -> lowering.lower (host, strings -> table)
                                    -> nodal_upload_components
                                    -> nodal_assemble_symbolic / _numeric  (HIP)
    Circuit.solve    -> nodal_solve_dense | nodal_solve_sparse            (HIP)

`Circuit.G` / `Circuit.A` are exported from the device on first access (numpy
array for the dense path, scipy CSR for the sparse path) so that code written
against the reference's attributes keeps working without paying a device->host
copy on the hot path.
"""

import contextlib
import logging
import os
import warnings

import numpy as np

from . import _ffi
from . import constants as c
from .lowering import lower
from .netlist import Netlist, UnconnectedCircuitError, is_connected

try:  # same warning class the reference's spsolve call emits
    from scipy.sparse.linalg import MatrixRankWarning
except Exception:  # pragma: no cover - scipy is optional at run time
    class MatrixRankWarning(UserWarning):
        pass


def _warn_singular(singular):
    """The reference's warning for a sparse system that is singular, attributed to the caller of the Circuit method
    that calls this (hence the stack level: this frame, the method, its caller)."""
    if singular:
        warnings.warn("Matrix is exactly singular", MatrixRankWarning, stacklevel=3)


def default_device():
    return int(os.environ.get("NODAL_DEVICE", os.environ.get("LOCAL_RANK", "0")))


# Device contexts are expensive to create (four HIP streams, one of them CU-masked, a dozen
# events: ~30 ms) and cheap to reuse (their buffers grow on demand), so a Circuit borrows one
# from this pool and hands it back when it is garbage collected.
# (The pool is touched from Circuit.__del__, i.e. from whatever thread the collector runs on, while the lanes of a
# long resistance sweep build Circuits on threads of their own (equiv.py): one lock around every look at it.  A
# re-entrant one: a collection triggered inside the locked region may run another Circuit's __del__ on this thread.)
import threading

_IDLE_HANDLES = {}
_MAX_IDLE = 4
_POOL_LOCK = threading.RLock()


def _acquire_handle(device):
    with _POOL_LOCK:
        idle = _IDLE_HANDLES.get(device)
        while idle:
            h = idle.pop()
            if not h.closed:
                return h
    return _ffi.Handle(device)


def _release_handle(device, h):
    if h is None or h.closed:
        return
    with _POOL_LOCK:
        idle = _IDLE_HANDLES.setdefault(device, [])
        if len(idle) < _MAX_IDLE:
            idle.append(h)
            return
    h.close()


class Circuit:
    """Builds the linear system G e = A of a Netlist on the GPU.

    Attributes: netlist, sparse, G, A, currents (reference nodal/nodal.py:306-311).
    """

    def __init__(self, netlist, sparse=False, device=None):
        if not isinstance(netlist, Netlist):
            raise TypeError("Input isn't a netlist")
        self.netlist = netlist
        self.sparse = sparse
        self._device = default_device() if device is None else device
        self._handle = None
        self._G = self._A = None
        self._transient_child = None
        self._transient_dc = None
        self._transient_nl_dc = None
        self._transient_record = None
        self._newton_child = None
        self._transistor_child = None
        self.currents = self.build_model()

    @classmethod
    def _clone_of(cls, other, table=None):
        """A second device context holding the same assembled system as `other` (no second lowering of the
        netlist): the lanes of a long equivalent-resistance sweep (equiv.py).  With `table`: that table in place of
        `other`'s -- the circuit with its companion resistors (transient())."""
        self = cls.__new__(cls)
        self.netlist, self.sparse, self._device = other.netlist, other.sparse, other._device
        self._handle = None
        self._G = self._A = None
        self._transient_child = None
        self._transient_dc = None
        self._transient_nl_dc = None
        self._transient_record = None
        self._newton_child = None
        self._transistor_child = None
        self.table = other.table if table is None else table
        self.currents = other.currents
        self._assemble(self.table)
        return self

    def __del__(self):
        try:
            handle, self._handle = self._handle, None
            _release_handle(self._device, handle)
        except Exception:  # interpreter shutdown
            pass

    # -- assembly ----------------------------------------------------------
    def build_model(self):
        """Lower the netlist, upload the component table and assemble G, A on
        the device (reference nodal/nodal.py:338-398).  Returns `currents`."""
        nl = self.netlist
        table = self._lower(nl)
        self.table = table
        if table.first_error is not None:
            row, exc, probe = table.first_error
            # the reference would have hit an earlier stamp collision first
            prefix = table.truncated(row + (1 if probe else 0))
            if prefix.ncomp:
                self._assemble(prefix)
            raise exc
        self._assemble(table)
        if getattr(nl, "_fast", False):
            if not nl._is_anom.any():  # (no branch unknowns: the names are not even looked at)
                return []
            return nl._name[nl._is_anom].tolist()
        comps = nl.components
        return [key for key in nl.component_keys if comps[key].type in c.NODE_TYPES_ANOM]

    @staticmethod
    def _lower(nl):
        if getattr(nl, "_fast", False):
            from . import fastparse
            try:
                return fastparse.lower_fast(nl)
            except fastparse.Irregular:
                nl._demote()
        return lower(nl)

    def _assemble(self, table):
        if self._handle is None:
            self._handle = _acquire_handle(self._device)
        h = self._handle
        h.upload(table)
        h.assemble_symbolic()
        status, bad = h.assemble_numeric(0)
        if status == _ffi.E_ZERO_RESISTANCE:
            raise ValueError("Model error: resistors can't have null resistance")
        if status == _ffi.E_STAMP_COLLISION:
            raise AssertionError  # the reference's bare `assert G[i, j] == 0`

    # -- reference attributes, exported lazily -------------------------------
    @property
    def G(self):
        if self._G is None:
            h = self._handle
            if self.sparse:
                indptr, indices, data, rhs = h.export_csr()
                import scipy.sparse as spsp
                self._G = spsp.csr_matrix((data, indices, indptr), shape=(h.n, h.n))
                # The reference stamps into a dok_matrix, which never stores an exact zero (a +g / -g
                # pair, a zero gain): its `G.tocsr()` has no such entries (reference nodal/nodal.py:
                # 396-397).  The device keeps them -- the pattern is the topology's, whatever the
                # values -- so they are dropped from the exported copy only.
                self._G.eliminate_zeros()
                self._A = rhs
            else:
                self._G, self._A = h.export_dense()
        return self._G

    @property
    def A(self):
        if self._A is None:
            self._A = self._handle.export_csr()[3]
        return self._A

    # -- the library's errors as the reference's exceptions --------------------------
    def _singular(self, look_at_connectivity=True):
        """The exception the reference raises for a singular dense system (reference nodal/nodal.py:313-336)."""
        if look_at_connectivity and not is_connected(self.netlist):
            logging.error("Model error: unconnected circuit")
            return UnconnectedCircuitError()
        logging.error("Model error: matrix is singular")
        return np.linalg.LinAlgError("Singular matrix")

    @contextlib.contextmanager
    def _reference_errors(self, missing=None, message="no solution: call solve() first"):
        """Around a call into the library: a NodalHipError becomes what the reference would have raised.  `missing`:
        the text by which an E_INVALID says that what the call reads is not on the device ("" for any E_INVALID; None:
        the call reads nothing of the kind) -- ValueError(message).  E_SINGULAR on the dense path: _singular().
        Everything else, and E_SINGULAR on the sparse path, is raised again as it is."""
        try:
            yield
        except _ffi.NodalHipError as exc:
            if missing is not None and exc.status == _ffi.E_INVALID and missing in str(exc):
                raise ValueError(message) from None
            if exc.status != _ffi.E_SINGULAR or self.sparse:
                raise
            raise self._singular()

    # -- solve ---------------------------------------------------------------
    def solve(self):
        """Solve G e = A on the device (reference nodal/nodal.py:313-336).

        Raises numpy.linalg.LinAlgError when the dense system is singular and
        the circuit is connected, UnconnectedCircuitError when it is not.  The
        sparse path does not raise on a matrix that is singular by construction
        (floating sub-network, loop of voltage sources, exact zero pivot of a
        small system): like the reference's spsolve call it warns
        (MatrixRankWarning) and returns NaNs.  A large general system whose
        iteration does not converge and that is not singular by construction
        raises NodalHipError (never a wrong answer)."""
        h = self._handle
        if self.sparse:
            e, info, self.iterations, self.relative_residual = h.solve_sparse()
            _warn_singular(info > 0)
        else:
            e, info = h.solve_dense()
            if info > 0:
                raise self._singular()
        return Solution(e, self.netlist, self.currents)

    def branches(self):
        """Voltage, current and absorbed power of every component for the last solve()'s solution, computed
        on the device (nodal_branches): a Branches (branches.py), arrays in the order of
        `netlist.component_keys`.  Raises ValueError when there is no solution on the device: before the
        first solve(), or after a solve_sources() (a sweep does not keep the single solve's solution)."""
        from .branches import Branches
        with self._reference_errors(missing=""):
            v, i, p, dissipated, absorbed = self._handle.branches()
        return Branches(self.netlist, v, i, p, dissipated, absorbed, table=self.table)

    def solve_sources(self, sources, branches=False, keep_solutions=True):
        """Solve the circuit for many settings of its independent sources at once.

        `sources` maps names of A / E components to sequences of M values (every sequence the same
        length).  Member m is the circuit with those components' values replaced by their m-th
        values; G is shared, so the members share one factorisation or one multigrid hierarchy on
        the device.  Returns a SourceSweep (sweep.py): `result` [M, K+B], `sw[m]` the Solution of
        member m, `info`, `scaled_residual`.  Singular networks behave as in solve(): the dense path
        raises LinAlgError / UnconnectedCircuitError once, the sparse path returns NaN rows with
        info > 0 and warns once.  The circuit itself (its table, G, A) is left as it was.

        branches=True adds `sw.envelope` (branches.Envelope): per component the largest |current| any solved
        member drives through it, per node the lowest and highest potential, each with a member that attains
        it, and the members' power totals -- accumulated on the device block by block.  With
        keep_solutions=False (needs branches=True) the members' solutions are not brought to the host at
        all: `sw.result` is None and the envelope is the answer."""
        from .sweep import SourceSweep, check_sweep_options, resolve_sources
        check_sweep_options(branches, keep_solutions)
        rows, values = resolve_sources(self.netlist, sources)
        h = self._handle
        M = values.shape[0]
        if M == 0:
            from .branches import Envelope
            return SourceSweep(np.zeros((0, h.n)) if keep_solutions else None, np.zeros(0, dtype=np.int32), np.zeros(0),
                               self.netlist, self.currents,
                               envelope=Envelope.empty(self.netlist, self.table.ncomp) if branches else None)
        env = None
        with self._reference_errors():
            if branches:
                x, info, resid, env = h.solve_sources_branches(rows, values, dense=not self.sparse,
                                                               keep_solutions=keep_solutions)
            else:
                x, info, resid = h.solve_sources(rows, values, dense=not self.sparse)
        _warn_singular((info > 0).any())
        if env is not None:
            from .branches import Envelope
            env = Envelope(self.netlist, env["current_absmax"], env["current_member"], env["potential_min"],
                           env["potential_min_member"], env["potential_max"], env["potential_max_member"],
                           env["power"][:, 0].copy(), env["power"][:, 1].copy())
        return SourceSweep(x, info, resid, self.netlist, self.currents, envelope=env)

    def sensitivities(self, outputs, adjoints=False):
        """Derivatives of chosen outputs of the last solve()'s solution with respect to the value of every
        component, by the adjoint method on the device (nodal_sensitivities): one solve with G^T per
        output, sixteen outputs to a block, and one pass over the component table per block.

        `outputs` is a sequence of ("e", node), ("v", node_plus, node_minus) or ("i", component)
        (sensitivity.resolve_outputs).  Returns a Sensitivities (sensitivity.py): `values` [M, ncomp] in
        the order of `netlist.component_keys`, `output_values` [M], `info`, `scaled_residual`, and with
        adjoints=True `adjoints` [M, K+B].  Raises ValueError when there is no solution on the device, as
        branches() does.  Singular networks behave as in solve_sources(): the dense path raises
        LinAlgError / UnconnectedCircuitError, the sparse path returns NaN rows with info > 0 and warns
        once.  The circuit itself -- its solution, table, G, A -- is left as it was."""
        from .sensitivity import Sensitivities, resolve_outputs
        outputs = list(outputs)
        kind, p, q2 = resolve_outputs(self.netlist, outputs)
        h = self._handle
        with self._reference_errors(missing="no solution"):
            values, y, lam, resid, info = h.sensitivities(kind, p, q2, dense=not self.sparse, adjoints=adjoints)
        _warn_singular((info > 0).any())
        return Sensitivities(self.netlist, outputs, values, y, info, resid, adjoints=lam, table=self.table)

    def gradient(self, cotangents, sources=None, solutions=None, adjoints=False):
        """The gradient of a scalar loss L of the solution with respect to the value of every component, by the
        adjoint method on the device (nodal_gradient): one solve with G^T per member, sixteen members to a block,
        and the per-row formulas summed over the members on the device -- one number per component comes down.

        Single solve: `cotangents` [K+B] = dL/dx for the last solve()'s solution; ValueError when there is none on
        the device, as branches() (or pass `solutions` [K+B], a solution kept from an earlier solve()).  Sweep, L = sum_m L_m(x_m): `sources` as passed to solve_sources, `solutions` the
        SourceSweep.result [M, K+B] and `cotangents` [M, K+B] = dL_m/dx_m; shapes that do not fit raise ValueError.
        Returns a Gradient (gradient.py): `values` [ncomp] in the order of `netlist.component_keys` -- the part of
        dL/dvalue that goes through the solution; a loss that reads the values themselves adds its own partial
        derivative -- `source_values` (name -> [M], member m's derivative with respect to its own swept value),
        `info`, `scaled_residual`, and with adjoints=True `adjoints` [M, K+B].  Singular networks behave as in
        sensitivities(): the dense path raises LinAlgError / UnconnectedCircuitError, the sparse path returns NaN
        with info > 0 and warns once.  The circuit itself -- its solution if any, table, G, A -- is left as it was."""
        from .gradient import Gradient, check_gradient_arguments
        h = self._handle
        cot, rows, x, columns = check_gradient_arguments(self.netlist, h.n, cotangents, sources, solutions)
        with self._reference_errors(missing="no solution"):
            values, gsrc, lam, resid, info = h.gradient(cot, dense=not self.sparse, rows=rows, solutions=x,
                                                        adjoints=adjoints)
        _warn_singular((info > 0).any())
        by_name = {name: gsrc[:, cols].sum(axis=1) for name, cols in columns.items()}
        return Gradient(self.netlist, values, by_name, info, resid, adjoints=lam, table=self.table)

    # -- new component values on the same topology ---------------------------------
    @property
    def values(self):
        """The value column in force, float64 [ncomp] in the order of `netlist.component_keys`: the lowered
        netlist's, or what the last set_values() put in its place."""
        return self.table.value

    def set_values(self, values):
        """Replace the value of every component and assemble G, A anew on the device, without parsing or lowering
        the netlist again (nodal_upload_values + nodal_assemble_numeric): the other half of an optimisation loop.

        `values` is float64 [ncomp] in the order of `netlist.component_keys`, in the units the table carries (what
        `Circuit.values` returns).  Errors are those of building the circuit: ValueError for a null resistance,
        AssertionError for a stamp collision, ZeroDivisionError for a resistor of value 0 that drives a CCVS /
        CCCS; after any of them the circuit keeps its previous values and stays usable.  The solution on the
        device and the cached G / A exports are dropped; `table`, and with it branches(), sensitivities(),
        gradient() and the sweeps, read the new values.  The Netlist itself is NOT touched: its components keep
        the values they were read with."""
        table = self.table
        new = np.array(values, dtype=np.float64)
        if new.shape != (table.ncomp,):
            raise ValueError(f"values must have shape ({table.ncomp},), not {new.shape}")
        if table.B > 0:
            drv = np.asarray(table.drv)
            driven = (drv >= 0) & ((np.asarray(table.c) >= 0) | (np.asarray(table.d) >= 0))
            if driven.any() and (new[drv[driven]] == 0).any():
                raise ZeroDivisionError("float division by zero")  # (as lowering.py, as the reference)
        h = self._handle
        h.upload_values(new[None, :])
        status, bad = h.assemble_numeric(0)
        if status != _ffi.OK:
            h.upload_values(np.asarray(table.value, dtype=np.float64)[None, :])
            h.assemble_numeric(0)
            if status == _ffi.E_ZERO_RESISTANCE:
                raise ValueError("Model error: resistors can't have null resistance")
            raise AssertionError  # the reference's bare `assert G[i, j] == 0`
        self._G = self._A = None
        self._transient_child = None  # (its matrix carried the old values)
        self._transient_dc = None
        self._transient_nl_dc = None
        self._transient_record = None
        self._newton_child = None
        self._transistor_child = None
        self.table = table.with_values(new)

    def thevenin(self, ports, sources=True):
        """The multiport Thevenin equivalent of the circuit seen from `ports`: a sequence of
        (node_plus, node_minus) labels or of single labels (that node against ground;
        ports.resolve_ports).  Returns a PortEquivalent (ports.py): `z` [P, P], the open-circuit
        impedance matrix with the independent sources switched off and the dependent ones in place,
        `v_oc` [P], the port voltages of the last solve()'s solution, `info`, `scaled_residual`, and
        from them norton(), loaded(resistances), rows() (the reduced netlist).  The P solves are those
        of solve_sources -- one factorisation or one multigrid hierarchy, sixteen ports to a block --
        and only P x P numbers come to the host (nodal_port_matrix).

        With sources=True there must be a solution on the device: ValueError otherwise, as branches().
        With sources=False `v_oc` is None and no solve is needed.  Singular networks behave as in
        solve_sources(): the dense path raises LinAlgError / UnconnectedCircuitError, the sparse path
        returns NaN columns with info > 0 and warns once.  The circuit itself -- its solution, table,
        G, A -- is left as it was."""
        from .ports import PortEquivalent, _as_pair, resolve_ports
        ports = [_as_pair(self.netlist, port) for port in ports]
        ia, ib = resolve_ports(self.netlist, ports)
        with self._reference_errors(missing="no solution"):
            z, v_oc, info, resid = self._handle.port_matrix(ia, ib, dense=not self.sparse, voc=bool(sources))
        _warn_singular((info > 0).any())
        return PortEquivalent(self.netlist, ports, z, v_oc, info, resid)

    def transient(self, capacitors, dt, steps, sources=None, probes=(), method="euler", initial=None, keep_every=0,
                  envelope=False, record=False, inductors=(), initial_currents=None, current_probes=(), diodes=(),
                  diode_probes=(), max_iter=50, reltol=1e-3, vntol=1e-6, abstol=1e-12, gmin=1e-12, transistors=(),
                  transistor_probes=()):
        """Step the circuit with capacitors through `steps` time steps of length `dt` on the device (nodal_transient).

        `capacitors` is a sequence of (name, farads, node_a, node_b) on nodes of the netlist; `sources` maps names of
        A / E components to sequences of `steps` values, entry k-1 in force at t_k = k dt (solve_sources' argument; a
        source that is not named keeps its netlist value); `probes` are (node_plus, node_minus) pairs or single labels
        against ground (thevenin's ports).  initial=None starts from the last solve()'s solution -- the DC operating
        point with the capacitors open; ValueError when there is none on the device, as branches() -- otherwise
        `initial` is a float64 [K+B] vector of which the potentials are read.  method is "euler" or "trapezoidal"
        (which needs the DC start: ValueError with `initial`).  keep_every=s > 0 brings the full solution of every
        s-th step down, envelope=True adds per node the lowest and highest potential over the steps and a step that
        attains each.  Returns a Transient (transient.py): `t`, `waveforms` [steps+1, P], `solutions`,
        `solution_steps`, `envelope`, `info`, `scaled_residual`, `iterations`.  record=True (backward Euler only:
        ValueError with "trapezoidal") keeps the states x_0 .. x_steps on the device for transient_gradient(), until the
        next transient() or set_values(); the results are the same bits either way.

        The matrix is that of the netlist with one companion resistor per capacitor, assembled on a second device
        context that is kept on the circuit, keyed by the capacitors, dt and method, until set_values(): a second call
        with the same key -- other sources, probes or steps -- repeats no analysis, hierarchy setup or factorisation.
        Singular networks behave as in solve_sources(): the dense path raises LinAlgError / UnconnectedCircuitError,
        the sparse path returns NaN steps with info > 0 and warns once.  The circuit itself -- its solution, table,
        G, A -- is left as it was.

        `inductors` is a sequence of (name, henries, node_a, node_b) on nodes of the netlist (nodal_transient_rlc); an
        inductor's current counts positive from node_a to node_b through it.  With inductors initial=None starts from
        the DC operating point in which every inductor is a short: the netlist with one zero-volt `E` row per inductor,
        solved once on a third device context kept on the circuit, keyed by the inductors' leads, until set_values().
        The circuit's own solve() is neither needed nor touched then.  With `initial`, `initial_currents` [L] are the
        inductors' currents at t_0 (None: zero; ValueError without `initial`).  `current_probes` names inductors whose
        currents are returned as `currents` [steps+1, Q]; `final_currents` [L] is the state after the last step, so
        that a run continues from `solutions[-1]` and `final_currents`.  ValueError for a loop of inductors alone
        (the DC start would be singular) and for record=True with inductors (their adjoint is not implemented); a DC
        start that is singular together with other components behaves as a singular solve().

        `diodes` is a sequence of (name, i_sat, n_vt, anode, cathode) as operating_point() takes it (nodal_transient_nl):
        every step is then solved by Newton's method on the device, with operating_point()'s linearisation, junction
        limiting and convergence test under `max_iter`, `reltol`, `vntol`, `abstol` and `gmin`; a diode has no memory, so
        the method changes the capacitors' and inductors' companions only.  Without `diodes` nothing changes: the same
        calls, the same bits.  With diodes initial=None starts from the NONLINEAR DC operating point -- capacitors open,
        inductors shorts, diodes in -- found by nodal_newton_dc on a further device context kept on the circuit, keyed by
        the inductors' and diodes' leads, until set_values(); solve() is neither needed nor touched.  A start that does
        not converge warns once (RuntimeWarning) and gives every step NaN with info 2.  The child's table holds the
        capacitors', inductors' and diodes' companion rows in that order and is keyed by the diodes' leads as well.
        `diode_probes` names diodes whose v and i(v) are returned as `diode_voltages` and `diode_currents` [steps+1, Q];
        `newton_iterations` and `matrix_updates` [steps] count a step's Newton iterations and those of them that
        assembled and factored (an iteration in which no junction's conductance moved by a bit re-uses the matrix);
        `final_junctions` [D] are the limited junction voltages after the last step.  A step whose Newton loop does not
        converge has info 2: it and every later step are NaN, and the run warns once (RuntimeWarning).  ValueError for
        record=True with diodes (the adjoint is not implemented), and operating_point()'s for the diodes and tolerances.

        `transistors` is a sequence of (name, "npn" | "pnp", i_s, beta_f, beta_r, n_vt, collector, base, emitter) as
        operating_point() takes it (nodal_transient_nl_bjt): bipolar transistors by the Ebers-Moll model in its
        transport form, stepped by the same Newton loop.  The two junctions of every transistor join the diodes behind
        the caller's, limiting, gmin and test included; the transport current is linearised at the junctions' limited
        voltages in every iteration, and a step has converged when no diode and no transport fails.  A transistor has
        no memory either: no charge storage, Early effect or resistances (a fixed junction capacitance is a `capacitors`
        entry).  `transistors` without `diodes` is legal.  initial=None then starts from the nonlinear DC point with the
        transistors in as well (nodal_newton_dc_bjt), on a clone keyed by the transports' leads too.  The child's table
        holds the capacitors', inductors', diodes' and junctions' companion rows and behind them two `GM` rows per
        transistor, and is keyed by the transports' leads and junction indices as well; its network is never passive:
        the dense panel (n <= 64) or the sparse LU, never the multigrid.  Such a run assembles in EVERY Newton
        iteration, `matrix_updates == newton_iterations`: a transconductance has no gmin floor, so its bits move whenever
        a junction voltage moves.  `transistor_probes` names transistors whose `junction_voltages` [steps+1, Q, 2]
        (forward, reverse) and `collector_currents`, `base_currents`, `emitter_currents` [steps+1, Q] (positive into the
        terminal, as operating_point() forms them) are returned; `final_junctions` then has D + 2 T entries, the
        junctions' last, while `diode_voltages`, `diode_currents` and `diode_probes` stay the caller's diodes.  ValueError
        as operating_point() raises for transistors, for a transistor with the name of a diode, for record=True with
        transistors, and for a `transistor_probes` name that is unknown or given twice.  Without `transistors` nothing
        changes: the same calls, the same bits."""
        from .ports import _as_pair, resolve_ports
        from .sweep import resolve_sources
        from .transient import (METHODS, Transient, TransientEnvelope, bjt_companion_table, check_diode_probes,
                                check_inductor_arguments, check_transient_arguments, check_transistor_probes,
                                companion_table, diode_companion_table, resolve_capacitors, resolve_inductors)
        h = self._handle
        self._transient_record = None  # (whatever an earlier call recorded: the device drops it as well)
        dt, steps, code, x0 = check_transient_arguments(dt, steps, method, initial, h.n)
        if record and code != METHODS["euler"]:
            raise ValueError('record=True needs method="euler": the adjoint of the trapezoidal rule is not implemented')
        keep_every = int(keep_every)
        if keep_every < 0:
            raise ValueError(f"keep_every must not be negative, not {keep_every}")
        names, farads, ca, cb = resolve_capacitors(self.netlist, capacitors)
        lnames, henries, la, lb = resolve_inductors(self.netlist, inductors)
        i0, cur_index = check_inductor_arguments(lnames, initial, initial_currents, current_probes)
        if record and len(lnames):
            raise ValueError("record=True with inductors: the adjoint of a run with inductors is not implemented")
        D, T = len(diodes), len(transistors)
        nonlinear = D > 0 or T > 0
        transports = None  # (the transports' leads, junction indices and i_s, with transistors)
        if nonlinear:
            from . import operating_point as op
            if record and T:
                raise ValueError("record=True with transistors: the adjoint of a run with transistors is not implemented")
            if record:
                raise ValueError("record=True with diodes: the adjoint of a run with diodes is not implemented")
            max_iter, reltol, vntol, abstol, gmin, _ = op.check_operating_point_arguments(max_iter, reltol, vntol, abstol,
                                                                                          gmin, None, h.n)
            if T:
                diodes = list(diodes)
                tnames, sign, junctions, ta, tb, junction, i_s = op.resolve_transistors(self.netlist, transistors, first=D)
                if set(tnames) & {d[0] for d in diodes if len(d) == 5}:
                    raise ValueError("A transistor has the name of a diode")
                dnames, i_sat, n_vt, da, db = op.resolve_diodes(self.netlist, diodes + junctions)
                transports = (ta, tb, junction, i_s)
            else:
                dnames, i_sat, n_vt, da, db = op.resolve_diodes(self.netlist, diodes)
            diode_index = check_diode_probes(dnames[:D], diode_probes)
        else:
            check_diode_probes((), diode_probes)
        transistor_index = check_transistor_probes(tnames if T else (), transistor_probes)
        rows, values = resolve_sources(self.netlist, sources if sources is not None else {})
        if len(rows) and values.shape[0] != steps:
            raise ValueError(f"Source waveforms must have {steps} values (one per step), not {values.shape[0]}")
        if not len(rows):
            values = np.zeros((steps, 0), dtype=np.float64)
        probes = [_as_pair(self.netlist, port) for port in probes]
        pa, pb = resolve_ports(self.netlist, probes)
        dc_singular = dc_lost = False
        if x0 is None and nonlinear:
            x0, i0, dc_singular, dc_lost = self._transient_nl_dc_start(la, lb, i_sat, n_vt, da, db, gmin, max_iter, reltol,
                                                                       vntol, abstol, transports)
        elif x0 is None and len(lnames):
            x0, i0, dc_singular = self._transient_dc_start(la, lb)
        elif x0 is None:
            with self._reference_errors(missing=""):
                x0 = h.download_x()
        key = (farads.tobytes(), ca.tobytes(), cb.tobytes(), dt, code)
        if len(lnames):
            key += (henries.tobytes(), la.tobytes(), lb.tobytes())
        if nonlinear:
            key += ("diodes", da.tobytes(), db.tobytes())
        if T:
            key += ("transistors", ta.tobytes(), tb.tobytes(), junction.tobytes())
        if self._transient_child is None or self._transient_child[0] != key:
            self._transient_child = None  # (its device context goes back to the pool first)
            diode_rows = None
            if T:
                table, cap_rows, ind_rows, diode_rows, gm_rows = bjt_companion_table(
                    self.table, farads, ca, cb, dt, code, henries, la, lb, i_sat, n_vt, da, db, ta, tb, junction, i_s, gmin)
            elif nonlinear:
                table, cap_rows, ind_rows, diode_rows = diode_companion_table(self.table, farads, ca, cb, dt, code, henries,
                                                                              la, lb, i_sat, n_vt, da, db, gmin)
            elif len(lnames):
                table, cap_rows, ind_rows = companion_table(self.table, farads, ca, cb, dt, code, henries, la, lb)
            else:
                (table, cap_rows), ind_rows = companion_table(self.table, farads, ca, cb, dt, code), None
            # (with transistors a sixth entry: the GM rows [T, 2])
            self._transient_child = (key, Circuit._clone_of(self, table), cap_rows, ind_rows, diode_rows) + ((gm_rows,) if T else ())
        _, child, cap_rows, ind_rows, diode_rows = self._transient_child[:5]
        ch = child._handle
        cur = final = junctions = None
        try:
            with self._reference_errors():
                if record:
                    ch.set_option(_ffi.OPT_TRANSIENT_TAPE, 1)
                if dc_singular or dc_lost:  # (sparse: the start is NaN, and with it every step)
                    wave = np.full((steps + 1, len(pa)), np.nan)
                    x = np.full((steps // keep_every, h.n), np.nan) if keep_every > 0 else None
                    env = None
                    if envelope:
                        K = self.table.K
                        env = {"potential_min": np.full(K, np.nan), "potential_min_step": np.full(K, -1, dtype=np.int32),
                               "potential_max": np.full(K, np.nan), "potential_max_step": np.full(K, -1, dtype=np.int32)}
                    resid, info, iters = np.full(steps, np.nan), np.ones(steps, dtype=np.int32), np.zeros(steps, dtype=np.int32)
                    cur, final = np.full((steps + 1, len(cur_index)), np.nan), np.full(len(lnames), np.nan)
                    if nonlinear:
                        info *= 1 if dc_singular else 2
                        junctions = {"newton": np.zeros(steps, dtype=np.int32), "updates": np.zeros(steps, dtype=np.int32),
                                     "v": np.full((steps + 1, len(diode_index)), np.nan),
                                     "i": np.full((steps + 1, len(diode_index)), np.nan), "vh": np.full(len(dnames), np.nan)}
                        if T:
                            junctions["tv"] = np.full((steps + 1, len(transistor_index), 2), np.nan)
                            junctions["ti"] = np.full((steps + 1, len(transistor_index), 3), np.nan)
                elif T:
                    wave, x, env, resid, info, iters, cur, final, junctions = ch.transient_nl_bjt(
                        cap_rows, ind_rows, diode_rows, i_sat, n_vt, gmin, self._transient_child[5], junction, i_s, rows, values,
                        x0, i0, pa, pb, cur_index, diode_index, transistor_index, dense=not self.sparse, max_iter=max_iter,
                        reltol=reltol, vntol=vntol, abstol=abstol, method=code, keep_every=keep_every, envelope=envelope)
                elif nonlinear:
                    wave, x, env, resid, info, iters, cur, final, junctions = ch.transient_nl(
                        cap_rows, ind_rows, diode_rows, i_sat, n_vt, gmin, rows, values, x0, i0, pa, pb, cur_index,
                        diode_index, dense=not self.sparse, max_iter=max_iter, reltol=reltol, vntol=vntol, abstol=abstol,
                        method=code, keep_every=keep_every, envelope=envelope)
                elif len(lnames):
                    wave, x, env, resid, info, iters, cur, final = ch.transient_rlc(
                        cap_rows, ind_rows, rows, values, x0, i0, pa, pb, cur_index, dense=not self.sparse, method=code,
                        keep_every=keep_every, envelope=envelope)
                else:
                    wave, x, env, resid, info, iters = ch.transient(cap_rows, rows, values, x0, pa, pb, dense=not self.sparse,
                                                                    method=code, keep_every=keep_every, envelope=envelope)
        finally:
            if record:
                ch.set_option(_ffi.OPT_TRANSIENT_TAPE, 0)  # (the handle goes back to a pool some day)
        singular = (info == 1).any() or dc_singular
        _warn_singular(singular)
        if (info == 2).any():
            first = int(np.argmax(info == 2)) + 1
            warnings.warn("transient: the DC start did not converge" if dc_lost else
                          f"transient: step {first} did not converge in {max_iter} Newton iterations", RuntimeWarning,
                          stacklevel=2)
        if record and not singular:
            from .sweep import _row_map
            from .transient_gradient import TransientRecord
            row_map, columns, at = _row_map(self.netlist), {}, 0
            for name in (sources or {}):  # (the order resolve_sources lays the rows out in)
                columns[name] = list(range(at, at + len(row_map[name])))
                at += len(row_map[name])
            self._transient_record = TransientRecord(child, dt, farads, cap_rows, columns, len(rows), steps, probes, pa, pb,
                                                     np.array(x0, dtype=np.float64), initial is None)
        if env is not None:
            env = TransientEnvelope(env["potential_min"], env["potential_min_step"], env["potential_max"],
                                    env["potential_max_step"])
        kept = np.arange(1, steps // keep_every + 1, dtype=np.int64) * keep_every if keep_every > 0 else None
        terminals = {}
        if T:
            # the terminal currents, positive INTO the terminal; a PNP's are an NPN's negated (operating_point())
            s_q = sign[transistor_index]
            i_f, i_r, i_t = (junctions["ti"][:, :, q] for q in range(3))
            terminals = dict(transistor_probes=transistor_probes, junction_voltages=junctions["tv"],
                             collector_currents=s_q * (i_t - i_r), base_currents=s_q * (i_f + i_r),
                             emitter_currents=-s_q * (i_t + i_f))
        return Transient(dt * np.arange(steps + 1, dtype=np.float64), wave, probes, info, resid, iters, solutions=x,
                         solution_steps=kept, envelope=env, timings=ch.timings(), currents=cur,
                         current_probes=current_probes, final_currents=final,
                         **({} if junctions is None else dict(
                             newton_iterations=junctions["newton"], matrix_updates=junctions["updates"],
                             diode_voltages=junctions["v"], diode_currents=junctions["i"], diode_probes=diode_probes,
                             final_junctions=junctions["vh"])), **terminals)

    def operating_point(self, diodes, sources=None, initial=None, max_iter=100, reltol=1e-3, vntol=1e-6, abstol=1e-12,
                        gmin=1e-12, keep_iterates=False, transistors=()):
        """The DC operating point of the circuit with diodes, by Newton's method on the device (nodal_newton_dc).

        `diodes` is a sequence of (name, i_sat, n_vt, anode, cathode) on nodes of the netlist: diode d carries
        i(v) = i_sat (exp(v / n_vt) - 1) + gmin v from anode to cathode at v = x(anode) - x(cathode), n_vt in volts
        (emission coefficient times thermal voltage).  `sources` maps names of A / E components to ONE value each, in
        force for this call (solve_sources' names and errors; a source that is not named keeps its netlist value);
        `initial` is a float64 [K+B] vector of which the potentials are read (None: zeros) -- `initial=previous.x`
        together with `sources` gives DC transfer curves and continuation in the caller's hands.  An iteration
        linearises every diode at its limited junction voltage, assembles and solves; SPICE's junction limiting
        (pnjlim) keeps the exponentials finite; it has converged when every diode has
        |v - vh| <= reltol max(|v|, |vh|) + vntol and |i(v) - ihat| <= reltol max(|i(v)|, |ihat|) + abstol, ihat the
        current its linearisation predicted.  Returns an OperatingPoint (operating_point.py): `x`, `voltages`,
        `currents`, `conductances` [D], `converged`, `iterations`, `history`, `scaled_residual`, `timings`,
        linearised() -- the small-signal circuit at this point for ac(), noise(), thevenin(sources=False) --
        gradient(cotangent) -- dL/d(every component value, i_sat, n_vt, gmin, the sources named here) of a loss L(x)
        through this point by one adjoint solve (nodal_newton_gradient); it is taken at the circuit's values in force
        when it is called, and its `operating_point_residual` is how a caller sees that they moved since -- and with
        keep_iterates=True `iterates` and `limited_voltages`.

        The matrix is that of the netlist with one companion resistor per diode, assembled on a second device context
        that is kept on the circuit, keyed by the diodes' leads, until set_values(): a second call with other sources,
        diode parameters, tolerances or `initial` repeats no symbolic work (`timings[1] == 0.0`).  A run that does not
        converge in max_iter iterations returns converged=False and warns once (RuntimeWarning).  Singular iterations
        behave as in solve_sources(): the dense path raises LinAlgError / UnconnectedCircuitError, the sparse path
        returns NaN with info > 0 in the history and warns once.  ValueError for unknown nodes, duplicate names or
        names of components, non-positive i_sat / n_vt, negative gmin / tolerances, max_iter < 1, and an `initial`
        that is not finite or of another shape.  No floating-point atomics: a repeated call gives the same bits.  The
        circuit itself -- its solution if any, table, G, A, what transient() and ac() keep -- is left as it was;
        solve() is neither needed nor touched.

        `transistors` is a sequence of (name, "npn" | "pnp", i_s, beta_f, beta_r, n_vt, collector, base, emitter):
        bipolar transistors by the Ebers-Moll model in its transport form (nodal_newton_dc_bjt) -- two junction diodes
        `name.be`, `name.bc` (`name.eb`, `name.cb` for a PNP) with i_sat = i_s / beta_f and i_s / beta_r, which join the
        call's diodes behind the caller's, limiting, gmin and test included, plus the transport current
        i_T = i_s (exp(v_be / n_vt) - exp(v_bc / n_vt)) from collector to emitter (a PNP: every direction reversed),
        linearised at the junctions' limited voltages and tested like a diode's current.  No Early effect, high
        injection, resistances or charge storage.  `diodes=()` is legal with transistors.  The result then carries
        `transistors`, `junction_voltages` [T, 2], `collector_currents`, `base_currents`, `emitter_currents` [T]
        (positive into the terminal) and `transconductances` [T, 2]; `diodes`, `voltages`, `currents`, `conductances`
        stay the caller's diodes; with keep_iterates `limited_voltages` has D + 2 T columns, the junctions' last; the
        history has `transistors_not_converged`; linearised() is the hybrid-pi model; gradient() raises ValueError (the
        adjoint with transistors is not implemented).  The companion child of such a call is a second one, keyed by
        the transports' leads as well; its network is never passive, so the iterations take the dense panel
        (n <= 64) or the sparse LU, never the multigrid.  ValueError as for diodes, for a kind other than
        the two, and for i_s, beta_f, beta_r or n_vt that is not positive and finite."""
        from .operating_point import (NewtonHistory, OperatingPoint, check_operating_point_arguments, resolve_diodes,
                                      resolve_transistors)
        from .sweep import _row_map, resolve_sources
        h = self._handle
        max_iter, reltol, vntol, abstol, gmin, x0 = check_operating_point_arguments(max_iter, reltol, vntol, abstol, gmin,
                                                                                    initial, h.n)
        diodes, transistors = list(diodes), list(transistors)
        D, T = len(diodes), len(transistors)
        tnames, sign, junctions, ta, tb, junction, i_s = resolve_transistors(self.netlist, transistors, first=D)
        if set(tnames) & {d[0] for d in diodes if len(d) == 5}:
            raise ValueError("A transistor has the name of a diode")
        names, i_sat, n_vt, ia, ib = resolve_diodes(self.netlist, diodes + junctions)
        setting = {}
        if sources is not None:
            if not hasattr(sources, "items"):
                raise TypeError("sources must map component names to values")
            setting = {name: [value] for name, value in sources.items()}
        rows, values = resolve_sources(self.netlist, setting)
        values = values[0] if len(rows) else np.zeros(0, dtype=np.float64)
        row_map, columns, at = _row_map(self.netlist) if setting else {}, {}, 0
        for name in setting:  # (the order resolve_sources lays the rows out in)
            columns[name] = list(range(at, at + len(row_map[name])))
            at += len(row_map[name])
        if T:
            child, diode_rows, gm_rows = self._transistor_companion(i_sat, n_vt, ia, ib, gmin, ta, tb, junction, i_s)
        else:
            child, diode_rows = self._newton_companion(i_sat, n_vt, ia, ib, gmin)
        ch = child._handle
        with self._reference_errors():
            if T:
                r = ch.newton_dc_bjt(diode_rows, i_sat, n_vt, gmin, gm_rows, junction, i_s, rows, values, x0,
                                     dense=not self.sparse, max_iter=max_iter, reltol=reltol, vntol=vntol, abstol=abstol,
                                     keep_iterates=keep_iterates)
            else:
                r = ch.newton_dc(diode_rows, i_sat, n_vt, gmin, rows, values, x0, dense=not self.sparse, max_iter=max_iter,
                                 reltol=reltol, vntol=vntol, abstol=abstol, keep_iterates=keep_iterates)
        singular = (r["info"] > 0).any()
        _warn_singular(singular)
        if not r["converged"] and not singular:
            warnings.warn(f"operating_point did not converge in {r['iterations']} iterations", RuntimeWarning, stacklevel=2)
        history = NewtonHistory(r["record"], r["info"], r["iters"], r["route"])
        if not T:
            return OperatingPoint(r["x"], names, r["v"], r["i"], r["g"], r["converged"], r["iterations"], history,
                                  timings=ch.timings(), iterates=r["iterates"], limited_voltages=r["vh"], circuit=self,
                                  leads=(ia, ib), i_sat=i_sat, n_vt=n_vt, gmin=gmin, source_rows=rows, source_values=values,
                                  source_columns=columns)
        # the terminal currents, positive INTO the terminal; a PNP's are an NPN's negated
        i_f, i_r, i_t = r["i"][D::2], r["i"][D + 1::2], r["it"]
        return OperatingPoint(r["x"], names[:D], r["v"][:D], r["i"][:D], r["g"][:D], r["converged"], r["iterations"],
                              history, timings=ch.timings(), iterates=r["iterates"], limited_voltages=r["vh"], circuit=self,
                              leads=(ia, ib), i_sat=i_sat, n_vt=n_vt, gmin=gmin, source_rows=rows, source_values=values,
                              source_columns=columns, transistors=tnames, junction_voltages=r["v"][D:].reshape(T, 2),
                              collector_currents=sign * (i_t - i_r), base_currents=sign * (i_f + i_r),
                              emitter_currents=-sign * (i_t + i_f),
                              transconductances=np.stack([r["gmf"], r["gmr"]], axis=1),
                              transport=(ta, tb, junction, r["g"][D:]))

    def _newton_companion(self, i_sat, n_vt, ia, ib, gmin):
        """Find or make the companion child for these leads: (the Circuit that holds this circuit's table with one
        companion `R` row per diode, those rows' indices).  Kept on the circuit under the diodes' leads until
        set_values(); other leads re-key it (the earlier child's device context goes back to the pool first)."""
        from .operating_point import companion_table
        key = (ia.tobytes(), ib.tobytes())
        if self._newton_child is None or self._newton_child[0] != key:
            self._newton_child = None
            table, diode_rows = companion_table(self.table, i_sat, n_vt, ia, ib, gmin)
            self._newton_child = (key, Circuit._clone_of(self, table), diode_rows)
        _, child, diode_rows = self._newton_child
        return child, diode_rows

    def _transistor_companion(self, i_sat, n_vt, ia, ib, gmin, ta, tb, junction, i_s):
        """_newton_companion for a call with transistors: (the Circuit that holds this circuit's table with one `R` row
        per diode, the junctions among them, and two `GM` rows per transport; the diode rows; the GM rows [T, 2]).  A
        child of its own, kept under the diodes' AND the transports' leads until set_values()."""
        from .operating_point import transistor_companion_table
        key = (ia.tobytes(), ib.tobytes(), ta.tobytes(), tb.tobytes(), junction.tobytes())
        if self._transistor_child is None or self._transistor_child[0] != key:
            self._transistor_child = None
            table, diode_rows, gm_rows = transistor_companion_table(self.table, i_sat, n_vt, ia, ib, ta, tb, junction, i_s,
                                                                    gmin)
            self._transistor_child = (key, Circuit._clone_of(self, table), diode_rows, gm_rows)
        _, child, diode_rows, gm_rows = self._transistor_child
        return child, diode_rows, gm_rows

    def _operating_point_gradient(self, op, x, cotangent, adjoints):
        """OperatingPoint.gradient on this circuit: the companion child for the result's leads (the one its run used,
        unless another operating_point call or set_values() came between: then it is re-keyed or made anew from the
        values in force), nodal_newton_gradient on it, and the pieces as an OperatingPointGradient."""
        from .operating_point import OperatingPointGradient
        ia, ib = op._leads
        child, diode_rows = self._newton_companion(op.i_sat, op.n_vt, ia, ib, op.gmin)
        ch = child._handle
        with self._reference_errors():
            r = ch.newton_gradient(diode_rows, op.i_sat, op.n_vt, op.gmin, op.source_rows, op.source_values, x, cotangent,
                                   dense=not self.sparse, adjoints=adjoints)
        _warn_singular(r["info"] > 0)
        by_name = {name: r["sources"][cols].sum() for name, cols in (op.source_columns or {}).items()}
        return OperatingPointGradient(self.netlist, r["grad"], op.diodes, r["i_sat"], r["n_vt"], r["gmin"], by_name,
                                      r["info"], r["resid"], r["op_resid"], adjoint=r["adjoint"], timings=ch.timings(),
                                      table=self.table, diode_i_sat=op.i_sat, diode_n_vt=op.n_vt)

    def _transient_dc_start(self, la, lb):
        """The DC operating point with every inductor a short, of the netlist's own source values: (x_0 [K+B], i_0 [L],
        singular).  Solved on a clone that holds the table with one zero-volt `E` row per inductor, kept with its
        solution under the inductors' leads.  Dense and singular: LinAlgError (whether the netlist alone is connected
        says nothing about this system); sparse and singular: NaN."""
        from .transient import dc_table
        key = (la.tobytes(), lb.tobytes())
        if self._transient_dc is None or self._transient_dc[0] != key:
            self._transient_dc = None  # (its device context goes back to the pool first)
            clone = Circuit._clone_of(self, dc_table(self.table, la, lb))
            dh = clone._handle
            if self.sparse:
                e, info = dh.solve_sparse()[:2]
            else:
                e, info = dh.solve_dense()
                if info > 0:
                    raise self._singular(look_at_connectivity=False)
            self._transient_dc = (key, clone, np.array(e, dtype=np.float64), info > 0)
        _, _, e, singular = self._transient_dc
        n = self.table.n
        # (an E row's branch unknown is the current into lead a out of the element: from a to b it is the negative)
        return e[:n].copy(), -e[n:], singular

    def _transient_nl_dc_start(self, la, lb, i_sat, n_vt, da, db, gmin, max_iter, reltol, vntol, abstol, transports=None):
        """The nonlinear DC operating point with capacitors open, every inductor a short and the diodes in, of the
        netlist's own source values: (x_0 [K+B], i_0 [L], singular, lost).  Newton's method (nodal_newton_dc) on a clone
        that holds dc_table's zero-volt `E` rows and, behind them, the diodes' companion rows; the clone is kept under
        the inductors' and diodes' leads, the iteration runs anew for every call (parameters and tolerances may differ;
        nothing symbolic is repeated).  Dense and singular: LinAlgError; sparse and singular: NaN and singular=True; not
        converged: lost=True, the caller's warning.  `transports` (ta, tb, junction, i_s): the transistors are in as well --
        the diodes hold their junctions, the clone's table the two `GM` rows per transport behind the diodes' rows
        (operating_point.transistor_companion_table), the loop is nodal_newton_dc_bjt and the key holds the transports'
        leads and junction indices too."""
        from . import operating_point as op
        from .transient import dc_table
        key = (la.tobytes(), lb.tobytes(), da.tobytes(), db.tobytes())
        if transports is not None:
            ta, tb, junction, i_s = transports
            key += ("transistors", ta.tobytes(), tb.tobytes(), junction.tobytes())
        if self._transient_nl_dc is None or self._transient_nl_dc[0] != key:
            self._transient_nl_dc = None  # (its device context goes back to the pool first)
            table = dc_table(self.table, la, lb) if len(la) else self.table
            if transports is not None:
                table, diode_rows, gm_rows = op.transistor_companion_table(table, i_sat, n_vt, da, db, ta, tb, junction, i_s,
                                                                           gmin)
                self._transient_nl_dc = (key, Circuit._clone_of(self, table), diode_rows, gm_rows)
            else:
                table, diode_rows = op.companion_table(table, i_sat, n_vt, da, db, gmin)
                self._transient_nl_dc = (key, Circuit._clone_of(self, table), diode_rows)
        clone, diode_rows = self._transient_nl_dc[1:3]
        none = np.zeros(0, dtype=np.int64), np.zeros(0), None
        try:
            if transports is not None:
                r = clone._handle.newton_dc_bjt(diode_rows, i_sat, n_vt, gmin, self._transient_nl_dc[3], junction, i_s, *none,
                                                dense=not self.sparse, max_iter=max_iter, reltol=reltol, vntol=vntol,
                                                abstol=abstol)
            else:
                r = clone._handle.newton_dc(diode_rows, i_sat, n_vt, gmin, *none, dense=not self.sparse, max_iter=max_iter,
                                            reltol=reltol, vntol=vntol, abstol=abstol)
        except _ffi.NodalHipError as exc:
            if exc.status != _ffi.E_SINGULAR or self.sparse:
                raise
            raise self._singular(look_at_connectivity=False) from None
        n = self.table.n
        e = np.array(r["x"], dtype=np.float64)
        singular = bool((r["info"] > 0).any())
        return e[:n].copy(), -e[n:], singular, not singular and not r["converged"]

    def transient_gradient(self, wave_cotangents, probes=None, adjoints=False):
        """The gradient of a scalar loss L of the probe waveforms of the last transient(..., record=True), by the adjoint
        method on the device (nodal_transient_gradient): the same time stepping run backwards with the transposed
        matrix, on the hierarchy or factors the forward run left -- about the cost of one more transient run.

        `wave_cotangents` [steps+1, P] = dL / d waveforms; `probes` as transient() takes them, None: those of the
        recorded call.  Returns a TransientGradient (transient_gradient.py): `values` [ncomp] in the order of
        `netlist.component_keys` -- with the DC start (initial=None) the derivative through that start is included,
        by Circuit.gradient of dL/dx_0 -- `capacitors` [C] = dL/dC, `source_values` (name -> [steps]), `initial` [K+B] =
        dL/dx_0, `info`, `scaled_residual`, `timings`, and with adjoints=True `adjoints` [steps, K+B].  ValueError without
        a recorded transient (none yet, a later transient() without record, or set_values() since), for cotangents of
        another shape or that are not finite.  Singular networks behave as in gradient().  A second call with other
        cotangents repeats no matrix work; the circuit, the record and the next transient() are left as they were."""
        from .ports import _as_pair, resolve_ports
        from .transient_gradient import NO_RECORD, TransientGradient, check_transient_gradient_arguments
        rec = self._transient_record
        pa, pb = ((), ()) if rec is None else (rec.pa, rec.pb)
        if rec is not None and probes is not None:
            pa, pb = resolve_ports(self.netlist, [_as_pair(self.netlist, port) for port in probes])
        cot = check_transient_gradient_arguments(rec, wave_cotangents, len(pa))  # (raises without a record)
        ch = rec.child._handle
        with self._reference_errors(missing="no recorded transient", message=NO_RECORD):
            grad, gsrc, gx0, lam, resid, info = ch.transient_gradient(rec.steps, rec.nsrc, pa, pb, cot,
                                                                      dense=not self.sparse, adjoints=adjoints)
        timings = ch.timings()
        _warn_singular((info > 0).any())
        ncomp = self.table.ncomp
        values = grad[:ncomp].copy()
        capacitors = -(rec.dt / rec.farads ** 2) * grad[rec.cap_rows]  # (the companion value is dt / C)
        start = np.zeros(ncomp)
        if rec.dc_start:  # x_0 = G^-1 A of this circuit: dL/dx_0 goes on through the single solve's adjoint
            start = np.array(self.gradient(gx0, solutions=rec.x0).values, dtype=np.float64)
            values += start
        by_name = {name: gsrc[:, cols].sum(axis=1) for name, cols in rec.columns.items()}
        return TransientGradient(values, capacitors, by_name, gx0, info, resid, adjoints=lam, timings=timings,
                                 start_values=start)

    def ac(self, frequencies, capacitors=(), inductors=(), sources=None, probes=(), current_probes=(), keep_every=0,
           peaks=False):
        """The steady state of the circuit with capacitors and inductors at each of `frequencies` (Hz), on the device
        (nodal_ac_sweep): the phasors x of (G + j B(w)) x = s, w = 2 pi f, one solve of the real system of twice the
        size per frequency.

        `capacitors` and `inductors` are sequences of (name, farads or henries, node_a, node_b) on nodes of the netlist,
        as transient() takes them; loops of inductors are legal here.  The excitation is small-signal: `sources` maps
        names of A / E components to complex amplitudes that stay constant over the sweep, and every independent source
        that is not named is off (None: all of them, and every result is zero); dependent sources stay in place.
        TypeError / KeyError / ValueError for bad names as solve_sources gives them.  `probes` are (node_plus,
        node_minus) pairs or single labels against ground (thevenin's ports); `current_probes` names capacitors or
        inductors whose currents are wanted, positive from node_a to node_b through the element.  keep_every=s > 0
        brings the full solution of every s-th frequency down, peaks=True adds per node the largest |potential| over the
        frequencies and a frequency index that attains it.  Returns an ACSweep (ac.py): `frequencies`, `omega`,
        `phasors` [F, P], `currents` [F, Q], `solutions`, `solution_indices`, `peaks`, `info`, `scaled_residual`,
        `timings`, magnitude_db(), phase_deg().

        The doubled system lives on a child of the circuit's own device context; its pattern and symbolic analysis are
        kept under the elements' kinds and leads: a second call with other values, frequencies, amplitudes or probes
        repeats neither (`timings[0] == 0.0`).  Singular networks behave as in solve_sources(): the dense path raises
        LinAlgError / UnconnectedCircuitError, the sparse path returns NaN rows with info > 0 for the singular
        frequencies and warns once.  The circuit itself -- its solution if any, table, G, A, a recorded transient -- is
        left as it was; solve() is neither needed nor touched."""
        from .ac import ACPeaks, ACSweep, check_ac_arguments, resolve_amplitudes, resolve_reactive
        from .ports import _as_pair, resolve_ports
        omega = check_ac_arguments(frequencies)
        keep_every = int(keep_every)
        if keep_every < 0:
            raise ValueError(f"keep_every must not be negative, not {keep_every}")
        names, kind, value, ea, eb = resolve_reactive(self.netlist, capacitors, inductors)
        rows, amplitudes = resolve_amplitudes(self.netlist, sources)
        probes = [_as_pair(self.netlist, port) for port in probes]
        pa, pb = resolve_ports(self.netlist, probes)
        index = {name: q for q, name in enumerate(names)}
        current_probes = list(current_probes)
        for name in current_probes:
            if name not in index:
                raise KeyError(f"current probe {name!r} is not the name of a capacitor or an inductor")
        cur_index = np.asarray([index[name] for name in current_probes], dtype=np.int32).reshape(len(current_probes))
        h = self._handle
        with self._reference_errors():
            wave, cur, x, peak, resid, info = h.ac_sweep(omega, kind, value, ea, eb, rows, amplitudes, pa, pb, cur_index,
                                                         dense=not self.sparse, keep_every=keep_every, peaks=peaks)
        timings = h.timings()
        _warn_singular((info > 0).any())
        kept = np.arange(1, len(omega) // keep_every + 1, dtype=np.int64) * keep_every - 1 if keep_every > 0 else None
        return ACSweep(np.array(frequencies, dtype=np.float64), omega, wave, probes, info, resid, currents=cur,
                       current_probes=current_probes, solutions=x, solution_indices=kept,
                       peaks=ACPeaks(peak[0], peak[1]) if peaks else None, timings=timings)

    def ac_ports(self, frequencies, ports, capacitors=(), inductors=(), peaks=False):
        """The impedance matrix Z(jw) of the circuit with capacitors and inductors seen from `ports`, at each of
        `frequencies` (Hz), on the device (nodal_ac_ports): Z[f][p][q] is the voltage of port p per ampere entering
        node_plus of port q and leaving its node_minus, with every independent source off and the dependent ones in
        place -- thevenin()'s `z` at a frequency, ac()'s matrix G + j B(w).

        `ports` are (node_plus, node_minus) pairs or single labels against ground, resolved as thevenin() resolves
        them; `capacitors` and `inductors` are sequences of (name, farads or henries, node_a, node_b) as ac() takes
        them.  KeyError / ValueError for bad labels, ports, values and frequencies as those two give them.  A port
        between a node and itself has a row and a column of exactly 0; two identical ports are legal.  peaks=True adds
        per node the largest |potential| per ampere over all ports and solved frequencies, with the port and the
        frequency index that attain it.  Returns an ACPortSweep (ac_ports.py): `frequencies`, `omega`, `ports`, `z`
        [F, P, P], `info` [F], `scaled_residual` [F, P], `peaks`, `work`, `timings`, driving_point(), reciprocity(),
        y(), s(z0), peak_impedance().

        A frequency costs ONE numeric factorisation whatever the number of ports; the ports go through the factors
        sixteen at a time and only F x P x P numbers come to the host.  The doubled system is the one ac() keeps on the
        circuit's device context: pattern and symbolic analysis are shared with ac() in either order, and with noise()
        wherever that shares with ac() (`timings[0] == 0.0`).  No floating-point atomics: a repeated call gives the
        same bits.  Singular networks behave as in ac(): the dense path raises LinAlgError / UnconnectedCircuitError,
        the sparse path returns NaN for the singular frequencies with info > 0 and warns once.  The circuit itself --
        its solution if any, table, G, A, a recorded transient, what ac() and noise() keep -- is left as it was;
        solve() is neither needed nor touched."""
        from .ac import resolve_reactive
        from .ac_ports import ACPortPeaks, ACPortSweep, check_ac_port_arguments
        omega, pairs, ia, ib = check_ac_port_arguments(self.netlist, frequencies, ports)
        _, kind, value, ea, eb = resolve_reactive(self.netlist, capacitors, inductors)
        h = self._handle
        with self._reference_errors():
            z, peak, resid, info, work = h.ac_ports(omega, kind, value, ea, eb, ia, ib, dense=not self.sparse, peaks=peaks)
        timings = h.timings()
        _warn_singular((info > 0).any())
        return ACPortSweep(np.array(frequencies, dtype=np.float64), omega, pairs, z, info, resid,
                           peaks=ACPortPeaks(*peak) if peaks else None, work=work, timings=timings)

    def noise(self, frequencies, capacitors=(), inductors=(), outputs=(), input=None, temperature=300.0,
              contributions=False):
        """The thermal noise of the circuit's resistors at each of `frequencies` (Hz), on the device (nodal_ac_noise):
        per output the density S_out(f) in V^2/Hz, summed over every resistor, from ONE adjoint solve per output and
        frequency, (G + j B(w))^T y = e(out+) - e(out-), instead of one solve per resistor.

        `capacitors` and `inductors` are sequences of (name, farads or henries, node_a, node_b) as ac() takes them, and
        G + j B(w) is the matrix of ac().  `outputs` are (node_plus, node_minus) pairs or single labels against ground,
        resolved as ac() resolves `probes`.  A table row of type R with a value > 0 and leads (a, b) adds
        4 k_B T / R |y(a) - y(b)|^2 to an output, `temperature` in kelvin for the whole network; sources, dependent
        elements, capacitors, inductors, resistors with a value <= 0 and resistors with both leads on one node are
        noiseless and add exactly 0.0.  `input` names one A or E component: the result then carries the gain
        H(f) = y^T s from that source (amplitude 1, every other independent source off, as in ac()) to each output and
        the input-referred density S_out / |H|^2.  TypeError / KeyError / ValueError for bad names and values as ac()
        gives them; ValueError for a temperature that is not finite and > 0 and for an `input` that names more than
        one row.  contributions=True adds every component's share integrated over the frequencies by the trapezoid
        rule, [P, ncomp] in the order of `netlist.component_keys` (the frequencies must then be strictly increasing);
        the sum is accumulated on the device, so the [F, P, ncomp] array never exists.  Returns a NoiseSweep
        (noise.py): `frequencies`, `omega`, `outputs`, `density` [F, P], `gain`, `input_density`, `contributions`,
        `info`, `scaled_residual` [F, P], `timings`, amplitude_density(), integrated(), rms(), top(p, count).

        No forward solution is needed or made, and a frequency costs one numeric factorisation whatever the number of
        outputs.  The transposed system lives on a child of the circuit's own device context, kept like ac()'s under the
        elements' kinds and leads: a second call with other values, frequencies, outputs or temperature repeats neither
        its pattern nor its symbolic analysis (`timings[0] == 0.0`), and a passive circuit without branch rows, whose
        matrix is symmetric, shares both with ac() in either order.  No floating-point atomics: a repeated call gives
        the same bits.  Singular networks behave as in ac(): the dense path raises LinAlgError /
        UnconnectedCircuitError, the sparse path returns NaN rows with info > 0 for the singular frequencies, NaN in
        every integrated quantity, and warns once.  The circuit itself -- its solution if any, table, G, A, a recorded
        transient, what ac() keeps -- is left as it was; solve() is neither needed nor touched."""
        from .ac import check_ac_arguments, resolve_amplitudes, resolve_reactive
        from .noise import NoiseSweep, check_noise_arguments, trapezoid_weights
        from .ports import _as_pair, resolve_ports
        omega = check_ac_arguments(frequencies)
        temperature = check_noise_arguments(temperature, contributions, frequencies)
        _, kind, value, ea, eb = resolve_reactive(self.netlist, capacitors, inductors)
        outputs = [_as_pair(self.netlist, port) for port in outputs]
        oa, ob = resolve_ports(self.netlist, outputs)
        input_row = -1
        if input is not None:
            if not isinstance(input, str):
                raise TypeError("input must be the name of one A or E component")
            rows, _ = resolve_amplitudes(self.netlist, {input: 1.0})
            if len(rows) != 1:
                raise ValueError(f"input {input!r} names {len(rows)} rows of the table, not one")
            input_row = int(rows[0])
        freqs = np.array(frequencies, dtype=np.float64)
        weight = trapezoid_weights(freqs) if contributions else None
        h = self._handle
        with self._reference_errors():
            density, gain, contrib, resid, info = h.ac_noise(omega, kind, value, ea, eb, temperature, oa, ob,
                                                             dense=not self.sparse, input_row=input_row, weight=weight)
        timings = h.timings()
        _warn_singular((info > 0).any())
        referred = None
        if gain is not None:
            with np.errstate(divide="ignore", invalid="ignore"):
                referred = density / (gain.real * gain.real + gain.imag * gain.imag)
        return NoiseSweep(freqs, omega, outputs, density, info, resid, gain=gain, input_density=referred,
                          contributions=contrib, names=list(self.netlist.component_keys) if contributions else None,
                          timings=timings)

    def ac_gradient(self, frequencies, cotangents, capacitors=(), inductors=(), sources=None, probes=(), adjoints=False):
        """The derivative of a real scalar loss L of ac()'s probe phasors with respect to every component value, every
        capacitance and inductance and every driven amplitude, on the device (nodal_ac_gradient): one forward and one
        adjoint solve per frequency, (G + j B(w))^T y = sum_p conj(g_p) (e(a_p) - e(b_p)), instead of two sweeps per
        parameter by central differences.

        `frequencies`, `capacitors`, `inductors`, `sources` and `probes` are those of ac(), with its errors.
        `cotangents` is complex [F, P]: g[f][p] = dL/dRe W[f][p] + j dL/dIm W[f][p] of the phasors W = ac(...).phasors --
        what torch's backward hands over for a complex tensor; for L = sum w |W - t|^2 it is 2 w (W - t).  TypeError
        for cotangents that are not complex, ValueError for another shape and for entries that are not finite.
        Returns an ACGradient (ac_gradient.py): `values` [ncomp] in the order of `netlist.component_keys` (exactly 0.0
        at A / E rows: the small-signal excitation never reads their table value), `capacitors`, `inductors` (and
        `capacitors_by_name`, `inductors_by_name`) with respect to the farads and henries as passed, `sources` name ->
        complex in the cotangents' convention, summed over the frequencies and the rows that carry the name,
        `source_terms` [F, R], `phasors` [F, P], `info`, `scaled_residual` [F, 2] (forward, adjoint), `adjoints`
        [F, K+B] with adjoints=True, `work`, `timings`.

        A circuit whose matrix is symmetric (passive, no branch rows) spends ONE numeric factorisation per frequency on
        both solves; any other spends two, the second on the transposed system noise() keeps.  Patterns and symbolic
        analyses are shared with ac(), noise() and ac_ports() in either order (`timings[0] == 0.0`).  The sums over the
        frequencies are formed on the device in ascending order without floating-point atomics: a repeated call gives
        the same bits.  Singular networks behave as in noise(): the dense path raises LinAlgError /
        UnconnectedCircuitError, the sparse path returns NaN rows with info > 0 for the singular frequencies, NaN in
        every summed gradient, and warns once.  The circuit itself -- its solution if any, table, G, A, a recorded
        transient, what ac(), noise() and ac_ports() keep -- is left as it was; solve() is neither needed nor
        touched."""
        from .ac import check_ac_arguments, resolve_amplitudes, resolve_reactive
        from .ac_gradient import ACGradient, check_ac_gradient_arguments, sources_by_name
        from .ports import _as_pair, resolve_ports
        omega = check_ac_arguments(frequencies)
        names, kind, value, ea, eb = resolve_reactive(self.netlist, capacitors, inductors)
        rows, amplitudes = resolve_amplitudes(self.netlist, sources)
        probes = [_as_pair(self.netlist, port) for port in probes]
        pa, pb = resolve_ports(self.netlist, probes)
        cot = check_ac_gradient_arguments(cotangents, len(omega), len(probes))
        h = self._handle
        with self._reference_errors():
            wave, grad, greact, gsrc, lam, resid, info, work = h.ac_gradient(
                omega, kind, value, ea, eb, rows, amplitudes, pa, pb, cot, dense=not self.sparse, adjoints=adjoints)
        timings = h.timings()
        _warn_singular((info > 0).any())
        ncap = int((kind == 0).sum())
        return ACGradient(grad, greact[:ncap], greact[ncap:], sources_by_name(list(self.netlist.component_keys), rows, gsrc),
                          gsrc, wave, info, resid, capacitor_names=names[:ncap], inductor_names=names[ncap:],
                          source_rows=rows, adjoints=lam, work=work, timings=timings)

    def scaled_residual(self):
        """||G x - A||_inf / (||G||_inf ||x||_inf + ||A||_inf) of the last
        solution, computed on the device."""
        return self._handle.residual()


class Solution:
    """Result of Circuit.solve(): `result[0:K]` node potentials in nodenum
    order, `result[K:K+B]` branch currents in anomnum order; printable
    (reference nodal/nodal.py:401-434)."""

    def __init__(self, result, netlist, currents):
        self.result = result
        self._netlist = netlist
        self.nums = netlist.nums
        self.currents = currents
        self.ground = netlist.ground

    # (the netlist's own dicts, as in the reference -- nodal/nodal.py:416-420 aliases them -- but looked at only when
    # somebody does: a natively read netlist builds them on first access)
    @property
    def nodenum(self):
        return self._netlist.nodenum

    @property
    def anomnum(self):
        return self._netlist.anomnum

    def __str__(self):
        # values as str(np.float64) prints them (shortest round-trip repr), names in
        # lexicographic string order: reference nodal/nodal.py:422-434.  tolist() +
        # repr() gives the same digits as formatting np.float64 one by one, without a
        # numpy scalar object per line.
        result = np.asarray(self.result, dtype=np.float64)
        lines = [f"Ground node: {self.ground}"]
        # a natively read netlist: the million "e(...)" lines by the host library, from the label blob (round 5; the
        # same text, tests/test_frontend.py)
        from . import fastparse
        block = fastparse.native_potential_lines(self._netlist, result) if len(result) >= 20000 else None
        values = None
        if block is not None:
            if block:
                lines.append(block)
        else:
            values = result.tolist()
            nodenum = self.nodenum
            lines += [f"e({name}) \t= {values[nodenum[name]]!r}" for name in sorted(nodenum)]
        offset, anomnum = self.nums["kcl"], self.anomnum
        if anomnum:
            if values is None:
                values = result.tolist()
            lines += [f"i({name}) \t= {values[offset + anomnum[name]]!r}" for name in sorted(anomnum)]
        return "\n".join(lines)
