"""The numpy restatement every port test is measured against (never product code).

G and A come from the oracle's build_model (through tests.sensitivity_reference.Reference: numpy.linalg.solve for small
systems, splu for large ones), and the definitions are evaluated here:

    port q = (a_q, b_q), either may be ground (index -1, potential +0.0)
    s_q = e(a_q) - e(b_q), zeros in the branch rows;  G x_q = s_q  (G itself, not G^T)
    Z[p][q] = x_q[a_p] - x_q[b_p]                V_oc[p] = x[a_p] - x[b_p],  G x = A

Bars: TOL is the project's normwise bar for a solution, and an entry of Z is the difference of two entries of one
column, each carrying that error: 2 TOL |x_q|_inf + 8 EPS (|x_q[a_p]| + |x_q[b_p]|); V_oc likewise with x.
"""
import numpy as np

from tests.sensitivity_reference import EPS, TOL, Reference, node_labels, table_of  # noqa: F401


def port_indices(nl, ports):
    """(ia, ib) of (node_plus, node_minus) labels: the test's own reading, from nodenum and the ground label"""
    def node(label):
        return -1 if label == nl.ground else nl.nodenum[label]
    return np.array([node(a) for a, _ in ports], dtype=int), np.array([node(b) for _, b in ports], dtype=int)


def small_ports(nl):
    """every node against ground, (first, last) and its reverse, a repeated port, (ground, ground), (node, node)"""
    labels = node_labels(nl)
    g = nl.ground
    ports = [(label, g) for label in labels] + [(g, g)]
    if labels:
        ports += [(labels[0], labels[-1]), (labels[-1], labels[0]), (labels[0], g),
                  (labels[-1], labels[-1])]
    return ports


def sample_ports(nl, count, seed):
    """a seeded sample of `count` ports; port 1 has a ground lead in front, port 2 is (node, same node)"""
    rng = np.random.default_rng(seed)
    labels = node_labels(nl)
    pick = lambda: labels[int(rng.integers(len(labels)))]  # noqa: E731
    ports = [(pick(), pick() if q % 3 else nl.ground) for q in range(count)]
    if count > 1:
        ports[1] = (nl.ground, pick())
    if count > 2:
        same = pick()
        ports[2] = (same, same)
    return ports


def grounded_ports(nl, count, seed):
    """`count` distinct nodes, each against ground"""
    rng = np.random.default_rng(seed)
    labels = node_labels(nl)
    return [(labels[int(k)], nl.ground) for k in rng.choice(len(labels), size=count, replace=False)]


def _lead(x, index):
    """x at the node indices, +0.0 for ground"""
    return np.append(np.asarray(x, dtype=np.float64), 0.0)[index]


class PortReference:
    """the columns x_q, Z, V_oc and their bars for one netlist and one list of ports.  `ref` is a Reference made with
    transposed=False (its LU is G's); one made with transposed=True gives the WRONG answer that test 4 wants missed."""

    def __init__(self, ref, ports):
        self.ref = ref
        self.ports = list(ports)
        nl = ref.nl
        self.ia, self.ib = port_indices(nl, self.ports)
        n = ref.table.K + ref.table.B
        count = len(self.ports)
        self.columns = np.zeros((count, n))
        for q in range(count):
            s = np.zeros(n)
            if self.ia[q] >= 0:
                s[self.ia[q]] += 1.0
            if self.ib[q] >= 0:
                s[self.ib[q]] -= 1.0
            if s.any():  # (an all-zero right-hand side: x_q = 0 exactly)
                self.columns[q] = ref.adjoint(s)
        self.z = np.zeros((count, count))
        self.z_bar = np.zeros((count, count))
        for q in range(count):
            xa, xb = _lead(self.columns[q], self.ia), _lead(self.columns[q], self.ib)
            self.z[:, q] = xa - xb
            self.z_bar[:, q] = 2 * TOL * np.abs(self.columns[q]).max(initial=0.0) + 8 * EPS * (np.abs(xa) + np.abs(xb))
        xa, xb = _lead(ref.x, self.ia), _lead(ref.x, self.ib)
        self.v_oc = xa - xb
        self.v_bar = 2 * TOL * np.abs(ref.x).max(initial=0.0) + 8 * EPS * (np.abs(xa) + np.abs(xb))

    def worst_miss(self, z):
        """max |z - Z| / bar over the entries with a positive bar"""
        off = np.abs(np.asarray(z) - self.z)
        with np.errstate(all="ignore"):
            return float(np.where(self.z_bar > 0, off / self.z_bar, 0.0).max(initial=0.0))

    def loaded(self, resistances):
        """port voltages with those load resistors, and cond_inf of the P x P system they come from"""
        m = np.eye(len(self.ports)) + self.z * (1.0 / np.asarray(resistances, dtype=np.float64))[None, :]
        return np.linalg.solve(m, self.v_oc), float(np.linalg.cond(m, np.inf))


def port_voltages(nl, x, ports):
    """x (a solution of netlist nl) read at the ports"""
    ia, ib = port_indices(nl, ports)
    return _lead(x, ia) - _lead(x, ib)
