"""misaka-net_amd -- MI355X-native batched executor for Misaka Net TIS networks.

The hot path (many independent /compute inputs through one node network) runs
in hand-written gfx950 HIP kernels behind the C ABI of include/mk.h; this
package is the host-side mirror of the reference's interface for that path.
Import name: ``misaka_net_amd`` (a symlink to this directory).
"""
from . import _native
from .network import (
    BatchResult,
    KEY_NONE,
    NO_INSTANCE,
    Network,
    NodeSpec,
    SessionDirectory,
    SessionSet,
    SessionSnapshot,
    TisParseError,
    directory_home,
    directory_slots,
    generate_inputs_device,
    group_requests_device,
    group_requests_tmp_bytes,
    tokenize,
    valu_probe_device,
)
from . import dist, master, networks

__all__ = [
    "BatchResult",
    "Network",
    "NodeSpec",
    "SessionDirectory",
    "SessionSet",
    "SessionSnapshot",
    "TisParseError",
    "KEY_NONE",
    "NO_INSTANCE",
    "directory_home",
    "directory_slots",
    "generate_inputs_device",
    "group_requests_device",
    "group_requests_tmp_bytes",
    "tokenize",
    "valu_probe_device",
    "networks",
    "dist",
    "master",
    "_native",
]
