"""MI355X-native modified-nodal-analysis solver with Nodal.py's Python API."""
__version__ = "1.3.0"
from .netlist import (  # noqa: F401
    Component,
    Netlist,
    UnconnectedCircuitError,
    build_opmodel,
    find_ground_node,
    is_connected,
)
from .circuit import Circuit, Solution  # noqa: E402,F401
from .branches import Branches, Envelope  # noqa: E402,F401
from .sensitivity import Sensitivities, resolve_outputs  # noqa: E402,F401
from .gradient import Gradient, check_gradient_arguments  # noqa: E402,F401
from .transient import Transient, TransientEnvelope, resolve_capacitors  # noqa: E402,F401
from .operating_point import NewtonHistory, OperatingPoint, resolve_diodes  # noqa: E402,F401
from .ac import ACPeaks, ACSweep, resolve_reactive  # noqa: E402,F401
from .noise import NoiseSweep, trapezoid_weights  # noqa: E402,F401
from .ac_ports import ACPortPeaks, ACPortSweep, check_ac_port_arguments  # noqa: E402,F401
from .ac_gradient import ACGradient, check_ac_gradient_arguments  # noqa: E402,F401
from .ports import PortEquivalent, resolve_ports  # noqa: E402,F401
