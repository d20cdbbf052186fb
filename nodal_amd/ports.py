"""Multiport Thevenin / Norton equivalents: what the network looks like from chosen ports.

A port is an ordered pair of nodes (node_plus, node_minus); either may be the ground node.  With the
circuit's independent sources switched off (the dependent ones stay: they are part of G),

    Z[p][q]   volts at port p per ampere entering node_plus of port q and leaving its node_minus
              (the sign of `equivalent_resistance` and of an `["a1", "A", "1", a, b]` row),
    V_oc[p]   the voltage of port p in the solved circuit, nothing connected from outside,

so that v = V_oc + Z i for any currents i driven into the ports from outside (Thevenin); Y = Z^-1 and
I_sc = Y V_oc are the Norton form.  With the reference the only way to it is one
`equivalent_resistance` per pair (reference nodal/equiv.py:31-61: a rebuild and a solve each,
resistive networks only, the diagonal number alone); `Circuit.thevenin` gets the whole matrix from
the solves of a source sweep -- one factorisation or one multigrid hierarchy, sixteen ports to a
block -- and reads the solutions at the port nodes on the device (`nodal_port_matrix`,
csrc/ports.hip): P x P numbers come down, not P x n.

`resolve_ports` -- labels to indices, argument checks -- needs no device, and `PortEquivalent` is a
plain container that can be built from arrays.
"""

import numpy as np


def _port_node(netlist, label):
    """index of a node among the unknowns, -1 for the ground node; KeyError (the text of
    equivalent_resistance) for a label the netlist does not have"""
    if label == netlist.ground:
        return -1
    if label in netlist.nodenum:
        return int(netlist.nodenum[label])
    text = str(label)
    if text == str(netlist.ground):
        return -1
    if text in netlist.nodenum:
        return int(netlist.nodenum[text])
    raise KeyError(f"Node `{label}` not found in netlist")


def _as_pair(netlist, port):
    if isinstance(port, (tuple, list)):
        if len(port) != 2:
            raise ValueError(f"Port {port!r} is not (node_plus, node_minus) or a single node")
        return port[0], port[1]
    return port, netlist.ground


def resolve_ports(netlist, ports):
    """The ports of Circuit.thevenin as the arrays nodal_port_matrix takes.

    `ports` is a sequence of (node_plus, node_minus) labels or of single labels (that node against
    ground).  Returns (ia, ib), int32 [P] each, -1 for the ground node.  Raises KeyError for a node
    the netlist does not have and ValueError for a malformed port."""
    pairs = [_as_pair(netlist, port) for port in ports]
    ia = [_port_node(netlist, a) for a, _ in pairs]
    ib = [_port_node(netlist, b) for _, b in pairs]
    as_i32 = lambda v: np.asarray(v, dtype=np.int32).reshape(len(v))  # noqa: E731
    return as_i32(ia), as_i32(ib)


class PortEquivalent:
    """Result of Circuit.thevenin.

    ports: the (node_plus, node_minus) labels; z [P, P]: the open-circuit impedance matrix; v_oc [P]:
    the open-circuit voltages (None when the equivalent was asked for without sources); info [P]: 0
    solved, > 0 singular (sparse path: column q of z is NaN); scaled_residual [P] of the solves
    G x_q = s_q, computed on the device.

    norton() and loaded() are P x P LAPACK calls on the host: O(P^3) on a matrix of a few kB to MB,
    nothing on the hot path (that is the P solves with the n x n matrix, on the device)."""

    def __init__(self, netlist, ports, z, v_oc, info, scaled_residual):
        self._netlist = netlist
        self.ports = [_as_pair(netlist, port) for port in ports]
        count = len(self.ports)
        self.z = np.asarray(z, dtype=np.float64).reshape(count, count)
        self.v_oc = None if v_oc is None else np.asarray(v_oc, dtype=np.float64).reshape(count)
        self.info = np.asarray(info, dtype=np.int32).reshape(count)
        self.scaled_residual = np.asarray(scaled_residual, dtype=np.float64).reshape(count)

    def __len__(self):
        return len(self.ports)

    def reciprocity(self):
        """max |Z - Z^T| / max |Z|: 0 (to rounding) for a network of resistors, not for one with
        dependent sources; 0.0 for an empty or all-zero Z."""
        if self.z.size == 0:
            return 0.0
        scale = np.abs(self.z).max()
        if scale == 0.0:
            return 0.0
        return float(np.abs(self.z - self.z.T).max() / scale)

    def norton(self):
        """(Y, I_sc): the short-circuit admittance matrix Y = Z^-1 and the short-circuit currents
        I_sc = Y V_oc (None without sources), so that the currents entering the ports from outside are
        i = Y v - I_sc.  numpy.linalg.inv on the host; LinAlgError when Z is singular (a port between
        a node and itself, two ports that are the same pair)."""
        y = np.linalg.inv(self.z)
        return y, (None if self.v_oc is None else y @ self.v_oc)

    def loaded(self, resistances):
        """The port voltages with a resistor of `resistances[p]` ohms across every port p (inf: left
        open): v = (I + Z diag(1 / R))^-1 V_oc.  One P x P solve on the host."""
        if self.v_oc is None:
            raise ValueError("no open-circuit voltages: the equivalent was made with sources=False")
        r = np.asarray(resistances, dtype=np.float64)
        if r.shape != (len(self.ports),):
            raise ValueError("one resistance per port")
        with np.errstate(divide="ignore"):
            g = np.where(np.isinf(r), 0.0, 1.0 / r)
        return np.linalg.solve(np.eye(len(self.ports)) + self.z * g[None, :], self.v_oc)

    def rows(self, prefix="eq"):
        """The reduced netlist of a reciprocal network seen from ground-referenced ports: rows that
        `Netlist.from_rows` accepts and that, attached to any external circuit at the port nodes,
        behave as the whole network does.  With Y = Z^-1: a resistor -1 / Y_ij between nodes i and j
        wherever |Y_ij| > 1e-9 max diag Y, a resistor 1 / g_i to ground wherever the row sum g_i of Y
        exceeds 1e-9 Y_ii in magnitude, and a current source I_sc[i] into node i wherever it is not
        zero.  Raises ValueError unless every port is (node, ground) with distinct nodes, every info
        is 0 and reciprocity() <= 1e-9 (a network with dependent sources has no such netlist)."""
        ground = self._netlist.ground
        nodes = [a for a, _ in self.ports]
        if any(b != ground for _, b in self.ports) or any(a == ground for a in nodes):
            raise ValueError("a reduced netlist needs ground-referenced ports (node, ground)")
        if len(set(nodes)) != len(nodes):
            raise ValueError("a reduced netlist needs distinct port nodes")
        if (self.info != 0).any():
            raise ValueError("a singular network has no reduced netlist")
        if not self.reciprocity() <= 1e-9:
            raise ValueError("the network is not reciprocal (Z differs from its transpose): no netlist of "
                             "resistors and sources reproduces it")
        count = len(nodes)
        if count == 0:
            return []
        y, i_sc = self.norton()
        top = np.abs(np.diag(y)).max()
        out = []
        for i in range(count):
            for j in range(i + 1, count):
                if abs(y[i, j]) > 1e-9 * top:
                    out.append([f"{prefix}r{i}_{j}", "R", repr(float(-1.0 / y[i, j])), nodes[i], nodes[j]])
        for i in range(count):
            g = float(y[i].sum())
            if abs(g) > 1e-9 * y[i, i]:
                out.append([f"{prefix}r{i}_g", "R", repr(float(1.0 / g)), nodes[i], ground])
        if i_sc is not None:
            for i in range(count):
                if i_sc[i] != 0.0:
                    out.append([f"{prefix}a{i}", "A", repr(float(i_sc[i])), nodes[i], ground])
        return out

    def __str__(self):
        lines = [f"Ports: {len(self.ports)}"]
        for p, (a, b) in enumerate(self.ports):
            text = f"port {p} ({a}, {b})"
            if self.v_oc is not None:
                text += f" \tV_oc = {float(self.v_oc[p])!r}"
            text += f" \tZ = {float(self.z[p, p])!r}"
            if self.info[p] > 0:
                text += " \t(singular)"
            lines.append(text)
        return "\n".join(lines)
