"""ctypes binding of libsdnroute.so (C ABI: include/sdnroute.h).

This is the only way the product reaches the route kernels; there is no CPU
fallback.  If the library is missing or no gfx950 device is visible the
calls fail loudly (:class:`NativeUnavailable` / :class:`SdnrError`).

PyTorch ROCm bundles its own ``libamdhip64.so.7``; when torch is importable
it is imported first so that this library binds to the same HIP runtime
(shared soname) and device pointers / streams can be exchanged with torch.
"""

import ctypes
import os
import threading

import numpy as np

__all__ = ["NativeUnavailable", "SdnrError", "library", "library_path",
           "Context", "DEVICE_PTRS", "TIMING", "UNREACHED", "DIST_INF", "TREE_NONE",
           "EXPORTED_SYMBOLS", "unpack_tree"]

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libsdnroute.so"

DEVICE_PTRS = 0x1
TIMING = 0x2
SAME_TABLES = 0x4        # route expansion: the previous call's parent / port tables
LOADS_TO_ROOT = 0x8      # sdnr_link_loads: per-destination next-hop rows
LOADS_SPLIT_HOP = 0x10   # sdnr_ecmp_link_loads: even split over a switch's next hops
LFA_LINK_ONLY = 0x20     # sdnr_lfa_tables: link-protecting alternates only
MCAST_TO_ROOT = 0x40     # sdnr_multicast_trees: per-destination next-hop rows
UNREACHED = -1
DIST_INF = 0xFFFF
TREE_NONE = 0xFFFFFFFF
COST_INF = 0xFFFFFFFF    # sdnr_cost_tables: no route
UTIL_MAX = 0xFFFFFFFE    # sdnr_widest_tables: the largest link utilisation
TREE_INT32 = 0           # int32 parents (sdnr_dfs_rows_affected)
TREE_PORT16 = 1          # parent | port << 16 (sdnr_dfs_tables_packed)
TREE_SLOT = 2            # parent | slot << 26 (sdnr_dfs_tables_slots)
ABI_VERSION = 1

# every entry point declared in include/sdnroute.h
EXPORTED_SYMBOLS = (
    "sdnr_abi_version", "sdnr_build_id", "sdnr_last_error", "sdnr_device_count", "sdnr_create",
    "sdnr_create_multi", "sdnr_device_list", "sdnr_destroy", "sdnr_set_stream", "sdnr_synchronize", "sdnr_graph_upload",
    "sdnr_graph_info", "sdnr_dfs_tables", "sdnr_dfs_tables_packed", "sdnr_dfs_tables_slots",
    "sdnr_dfs_tables_tree", "sdnr_tree_pack", "sdnr_shortest_tables", "sdnr_route_expand_packed",
    "sdnr_apsp", "sdnr_route_offsets", "sdnr_route_expand", "sdnr_ecmp_counts",
    "sdnr_ecmp_routes",
    "sdnr_last_kernel_ms", "sdnr_last_kernel", "sdnr_last_launches", "sdnr_last_sweeps",
    "sdnr_edge_ports", "sdnr_dfs_rows_affected", "sdnr_link_loads",
    "sdnr_ecmp_link_loads", "sdnr_graph_costs", "sdnr_cost_tables",
    "sdnr_cost_ecmp_link_loads", "sdnr_graph_twin_reps", "sdnr_last_dfs_searched",
    "sdnr_last_dfs_form", "sdnr_last_dfs_quotient",
    "sdnr_failure_ecmp_link_loads", "sdnr_lfa_tables", "sdnr_whatif_ecmp_link_loads",
    "sdnr_widest_tables", "sdnr_fair_rates", "sdnr_ecmp_fair_rates", "sdnr_multicast_trees",
    "sdnr_last_grid", "sdnr_frr_link_loads", "sdnr_last_frr_items", "sdnr_fair_times",
    "sdnr_ecmp_fair_times", "sdnr_remote_lfa",
)


class NativeUnavailable(RuntimeError):
    """libsdnroute.so could not be loaded (not built, or no HIP runtime)."""


class SdnrError(RuntimeError):
    def __init__(self, code, msg):
        super(SdnrError, self).__init__("sdnroute error %d: %s" % (code, msg))
        self.code = code


_lib = None
_lock = threading.Lock()


def library_path():
    return os.environ.get("SDNROUTE_LIB", os.path.join(_HERE, _LIB_NAME))


def _bind(L):
    c_int, i32, u32, vp = ctypes.c_int, ctypes.c_int32, ctypes.c_uint32, ctypes.c_void_p
    sig = {
        "sdnr_abi_version": ([], c_int),
        "sdnr_build_id": ([], ctypes.c_char_p),
        "sdnr_last_error": ([], ctypes.c_char_p),
        "sdnr_device_count": ([ctypes.POINTER(c_int)], c_int),
        "sdnr_create": ([c_int, ctypes.POINTER(vp)], c_int),
        "sdnr_create_multi": ([ctypes.POINTER(c_int), c_int, ctypes.POINTER(vp)], c_int),
        "sdnr_device_list": ([vp, ctypes.POINTER(c_int), c_int, ctypes.POINTER(c_int)], c_int),
        "sdnr_destroy": ([vp], c_int),
        "sdnr_set_stream": ([vp, vp], c_int),
        "sdnr_synchronize": ([vp], c_int),
        "sdnr_graph_upload": ([vp, i32, i32, vp, vp, vp], c_int),
        "sdnr_graph_info": ([vp, ctypes.POINTER(i32), ctypes.POINTER(i32),
                             ctypes.POINTER(i32)], c_int),
        "sdnr_dfs_tables": ([vp, vp, i32, vp, vp, vp, u32], c_int),
        "sdnr_dfs_tables_packed": ([vp, vp, i32, vp, u32], c_int),
        "sdnr_dfs_tables_slots": ([vp, vp, i32, vp, u32], c_int),
        "sdnr_tree_pack": ([vp, vp, vp, ctypes.c_int64, vp, i32, u32], c_int),
        "sdnr_dfs_tables_tree": ([vp, vp, i32, vp, vp, i32, i32, u32], c_int),
        "sdnr_route_expand_packed": ([vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, u32], c_int),
        "sdnr_shortest_tables": ([vp, vp, i32, vp, vp, vp, u32], c_int),
        "sdnr_apsp": ([vp, vp, u32], c_int),
        "sdnr_route_offsets": ([vp, vp, i32, vp, vp, i32, vp, u32], c_int),
        "sdnr_ecmp_counts": ([vp, vp, i32, vp, u32], c_int),
        "sdnr_ecmp_routes": ([vp, vp, vp, i32, vp, vp, vp, i32, i32, vp, u32], c_int),
        "sdnr_route_expand": ([vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, u32], c_int),
        "sdnr_last_kernel_ms": ([vp, ctypes.POINTER(ctypes.c_float)], c_int),
        "sdnr_last_kernel": ([vp], ctypes.c_char_p),
        "sdnr_last_launches": ([vp, ctypes.POINTER(i32)], c_int),
        "sdnr_last_grid": ([vp, ctypes.POINTER(ctypes.c_int64)], c_int),
        "sdnr_last_sweeps": ([vp, ctypes.POINTER(i32)], c_int),
        "sdnr_edge_ports": ([vp, vp, i32, vp, i32, vp, u32], c_int),
        "sdnr_dfs_rows_affected": ([vp, vp, vp, i32, i32, i32, vp, vp, i32, i32, vp, u32], c_int),
        "sdnr_link_loads": ([vp, vp, i32, i32, vp, vp, vp, vp, u32], c_int),
        "sdnr_ecmp_link_loads": ([vp, vp, i32, vp, vp, vp, vp, u32], c_int),
        "sdnr_multicast_trees": ([vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                  u32], c_int),
        "sdnr_graph_costs": ([vp, vp], c_int),
        "sdnr_cost_tables": ([vp, vp, i32, vp, vp, vp, u32], c_int),
        "sdnr_cost_ecmp_link_loads": ([vp, vp, i32, vp, vp, vp, vp, u32], c_int),
        "sdnr_failure_ecmp_link_loads": ([vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, u32],
                                         c_int),
        "sdnr_lfa_tables": ([vp, vp, vp, i32, vp, vp, vp, vp, u32], c_int),
        "sdnr_whatif_ecmp_link_loads": ([vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp,
                                         vp, vp, u32], c_int),
        "sdnr_widest_tables": ([vp, vp, vp, vp, i32, vp, vp, vp, u32], c_int),
        "sdnr_fair_rates": ([vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp,
                             ctypes.POINTER(i32), u32], c_int),
        "sdnr_ecmp_fair_rates": ([vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp,
                                  ctypes.POINTER(i32), u32], c_int),
        "sdnr_fair_times": ([vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp,
                             i32, vp, ctypes.POINTER(i32), u32], c_int),
        "sdnr_ecmp_fair_times": ([vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp,
                                  i32, vp, ctypes.POINTER(i32), u32], c_int),
        "sdnr_graph_twin_reps": ([vp, vp], c_int),
        "sdnr_last_dfs_searched": ([vp, ctypes.POINTER(i32)], c_int),
        "sdnr_last_dfs_form": ([vp, ctypes.POINTER(i32)], c_int),
        "sdnr_last_dfs_quotient": ([vp, ctypes.POINTER(i32)], c_int),
        "sdnr_frr_link_loads": ([vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp,
                                 u32], c_int),
        "sdnr_last_frr_items": ([vp, ctypes.POINTER(ctypes.c_int64)], c_int),
        "sdnr_remote_lfa": ([vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, u32], c_int),
    }
    # an A/B build named by SDNROUTE_LIB may predate some entry points: those
    # stay unbound (calling one raises AttributeError); the in-tree library
    # must export every one
    older_ok = "SDNROUTE_LIB" in os.environ
    for name, (args, res) in sig.items():
        if older_ok and not hasattr(L, name):
            continue
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    return L


def library():
    """Load (once) and return the bound library."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = library_path()
        if not os.path.exists(path):
            raise NativeUnavailable(
                "%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "in the repository root" % path)
        try:   # share torch's HIP runtime when torch is around
            import torch  # noqa: F401
        except Exception:   # noqa: BLE001 - torch is optional plumbing
            pass
        try:
            L = ctypes.CDLL(path)
        except OSError as e:
            raise NativeUnavailable("cannot load %s: %s" % (path, e))
        _bind(L)
        if L.sdnr_abi_version() != ABI_VERSION:
            raise NativeUnavailable("ABI mismatch: library %d, binding %d"
                                    % (L.sdnr_abi_version(), ABI_VERSION))
        if "SDNROUTE_LIB" not in os.environ:     # A/B and diagnostic builds are named explicitly
            verify_build(L)
        _lib = L
        return L


def verify_build(L, csrc=None, include=None):
    """Refuse a library that was not built from the tree beside it: its
    sdnr_build_id() must equal the SHA-256 of the current sources, headers
    and flags (_buildinfo.tree_build_id).  Skipped when the sources are not
    there (a package installed without csrc/)."""
    from . import _buildinfo as B
    want = B.tree_build_id(csrc or B.CSRC, include or B.INCLUDE)
    if want is None:
        return
    got = L.sdnr_build_id().decode("ascii", "replace")
    if got != want:
        raise NativeUnavailable(
            "stale %s: built from sources %s, the tree is %s -- rebuild with "
            "`python -c 'import __graft_entry__ as g; g.build()'`" % (library_path(), got[:16],
                                                                    want[:16]))


def _check(rc):
    if rc != 0:
        msg = library().sdnr_last_error().decode("utf-8", "replace")
        raise SdnrError(rc, msg)


def device_count():
    n = ctypes.c_int(0)
    _check(library().sdnr_device_count(ctypes.byref(n)))
    return n.value


def unpack_tree(tree):
    """Packed tree rows -> (parent, port) int32, -1 where the packed half is
    0xFFFF (unreached vertex / the root's port)."""
    t = np.asarray(tree, np.uint32)
    parent = (t & 0xFFFF).astype(np.int32)
    port = (t >> 16).astype(np.int32)
    parent[parent == 0xFFFF] = -1
    port[port == 0xFFFF] = -1
    return parent, port


def unpack_slots(tree, csr):
    """Slot tree rows (parent | slot << 26) -> (parent, port) int32 with the
    CSR's port of each tree link; -1 for unreached vertices and the root's
    port."""
    t = np.asarray(tree, np.uint32)
    none = t == TREE_NONE
    parent = (t & 0x3FFFFFF).astype(np.int64)
    slot = (t >> 26).astype(np.int64)
    root = slot == 63
    rp = np.asarray(csr.row_ptr, np.int64)
    idx = np.where(none | root, 0, rp[np.where(none, 0, parent)] + slot)
    port = np.asarray(csr.port, np.int32)[idx]
    port[none | root] = -1
    parent = parent.astype(np.int32)
    parent[none] = -1
    return parent, port


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _p(address):
    """A device or host address as a nullable pointer argument: 0 is NULL."""
    return ctypes.c_void_p(address) if address else None


class Context(object):
    """A route-engine context (owns graph + scratch) on one HIP device, or --
    ``device`` a sequence -- over several (sdnr_create_multi: the table calls
    are sharded by source/destination over the devices, device-pointer
    buffers live on the first one)."""

    def __init__(self, device=0):
        self._lib = library()
        h = ctypes.c_void_p()
        if isinstance(device, (list, tuple)):
            devs = [int(d) for d in device]
            arr = (ctypes.c_int * len(devs))(*devs)
            _check(self._lib.sdnr_create_multi(arr, len(devs), ctypes.byref(h)))
            self.devices = devs
        else:
            _check(self._lib.sdnr_create(int(device), ctypes.byref(h)))
            self.devices = [int(device)]
        self._h = h
        self.device = self.devices[0]
        self.V = -1
        self.E = 0

    def device_list(self):
        n = ctypes.c_int()
        _check(self._lib.sdnr_device_list(self._h, None, 0, ctypes.byref(n)))
        arr = (ctypes.c_int * n.value)()
        _check(self._lib.sdnr_device_list(self._h, arr, n.value, ctypes.byref(n)))
        return list(arr)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sdnr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001 - interpreter shutdown
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- setup --------------------------------------------------------
    def set_stream(self, stream_handle):
        _check(self._lib.sdnr_set_stream(self._h, ctypes.c_void_p(stream_handle or 0)
                                         if stream_handle else None))

    def synchronize(self):
        _check(self._lib.sdnr_synchronize(self._h))

    def upload(self, csr):
        rp = np.ascontiguousarray(csr.row_ptr, np.int32)
        col = np.ascontiguousarray(csr.col, np.int32)
        port = np.ascontiguousarray(csr.port, np.int32)
        V, E = int(rp.shape[0] - 1), int(col.shape[0])
        _check(self._lib.sdnr_graph_upload(self._h, V, E, _ptr(rp),
                                           _ptr(col) if E else None,
                                           _ptr(port) if E else None))
        self.V, self.E = V, E

    def info(self):
        V, E, D = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _check(self._lib.sdnr_graph_info(self._h, ctypes.byref(V), ctypes.byref(E),
                                         ctypes.byref(D)))
        return V.value, E.value, D.value

    # -- host-buffer (synchronous) calls ------------------------------
    def dfs_tables(self, srcs, with_hops=True):
        srcs = np.ascontiguousarray(srcs, np.int32)
        S, V = int(srcs.shape[0]), self.V
        parent = np.empty((S, V), np.int32)
        port = np.empty((S, V), np.int32)
        hops = np.empty((S, V), np.int32) if with_hops else None
        _check(self._lib.sdnr_dfs_tables(self._h, _ptr(srcs), S, _ptr(parent),
                                         _ptr(port), _ptr(hops), 0))
        return parent, port, hops

    def dfs_tables_packed(self, srcs):
        """Packed trees: uint32 [S, V], parent | port << 16 (see unpack_tree)."""
        srcs = np.ascontiguousarray(srcs, np.int32)
        S, V = int(srcs.shape[0]), self.V
        tree = np.empty((S, V), np.uint32)
        _check(self._lib.sdnr_dfs_tables_packed(self._h, _ptr(srcs), S, _ptr(tree), 0))
        return tree

    def dfs_tables_slots(self, srcs):
        """Slot trees: uint32 [S, V], parent | slot << 26 (see unpack_slots)."""
        srcs = np.ascontiguousarray(srcs, np.int32)
        S, V = int(srcs.shape[0]), self.V
        tree = np.empty((S, V), np.uint32)
        _check(self._lib.sdnr_dfs_tables_slots(self._h, _ptr(srcs), S, _ptr(tree), 0))
        return tree

    def shortest_tables(self, dsts, with_nexthop=True):
        dsts = np.ascontiguousarray(dsts, np.int32)
        D, V = int(dsts.shape[0]), self.V
        dist = np.empty((D, V), np.uint16)
        nh = np.empty((D, V), np.int32) if with_nexthop else None
        nhp = np.empty((D, V), np.int32) if with_nexthop else None
        _check(self._lib.sdnr_shortest_tables(self._h, _ptr(dsts), D, _ptr(dist),
                                              _ptr(nh), _ptr(nhp), 0))
        return dist, nh, nhp

    def set_link_costs(self, cost):
        """Per-link costs of the uploaded graph (uint32 [E], CSR edge order,
        every one >= 1; None clears them): sdnr_graph_costs.  A new upload
        clears them too."""
        if cost is None:
            _check(self._lib.sdnr_graph_costs(self._h, None))
            return
        c = np.ascontiguousarray(cost, np.uint32)
        if c.shape != (self.E,):
            raise ValueError("one cost per link of the uploaded graph (%d)" % self.E)
        _check(self._lib.sdnr_graph_costs(self._h, _ptr(c)))

    def cost_tables(self, dsts, with_nexthop=True):
        """Least-cost tables under the uploaded costs: (pcost uint32 [D, V],
        nh, nh_port int32 or None), see sdnr_cost_tables."""
        dsts = np.ascontiguousarray(dsts, np.int32)
        D, V = int(dsts.shape[0]), self.V
        pcost = np.empty((D, V), np.uint32)
        nh = np.empty((D, V), np.int32) if with_nexthop else None
        nhp = np.empty((D, V), np.int32) if with_nexthop else None
        _check(self._lib.sdnr_cost_tables(self._h, _ptr(dsts), D, _ptr(pcost), _ptr(nh),
                                          _ptr(nhp), 0))
        return pcost, nh, nhp

    def widest_tables(self, pcost, util, dsts, with_nexthop=True):
        """Least-loaded tables inside the least-cost DAG: (bott uint32 [D, V],
        nh, nh_port int32 or None) from the pcost rows of ``dsts`` (uint32
        [D, V], cost_tables') and the link utilisations ``util`` (uint32 [E],
        CSR edge order), see sdnr_widest_tables."""
        dsts = np.ascontiguousarray(dsts, np.int32)
        D, V = int(dsts.shape[0]), self.V
        pcost = np.ascontiguousarray(pcost, np.uint32)
        util = np.ascontiguousarray(util, np.uint32)
        if pcost.shape != (D, V) or util.shape != (self.E,):
            raise ValueError("pcost is [len(dsts), V] (%d, %d), util one word per link (%d)"
                             % (D, V, self.E))
        bott = np.empty((D, V), np.uint32)
        nh = np.empty((D, V), np.int32) if with_nexthop else None
        nhp = np.empty((D, V), np.int32) if with_nexthop else None
        _check(self._lib.sdnr_widest_tables(self._h, _ptr(pcost), _ptr(util), _ptr(dsts), D,
                                            _ptr(bott), _ptr(nh), _ptr(nhp), 0))
        return bott, nh, nhp

    def expand_routes(self, parent, port, hops, rows, dsts, last_port):
        """Flow entries of many pairs from host tables: (offsets int64
        [n+1], hop_switch int32, hop_port int32); see sdnr_route_expand."""
        parent = np.ascontiguousarray(parent, np.int32)
        port = np.ascontiguousarray(port, np.int32)
        hops = np.ascontiguousarray(hops, np.int32)
        rows = np.ascontiguousarray(rows, np.int32)
        dsts = np.ascontiguousarray(dsts, np.int32)
        last = np.ascontiguousarray(last_port, np.int32)
        n, nrows = int(rows.shape[0]), int(parent.shape[0])
        off = np.empty(n + 1, np.int64)
        _check(self._lib.sdnr_route_offsets(self._h, _ptr(hops), nrows, _ptr(rows), _ptr(dsts),
                                            n, _ptr(off), 0))
        total = int(off[-1])
        sw = np.empty(total, np.int32)
        hp = np.empty(total, np.int32)
        _check(self._lib.sdnr_route_expand(self._h, _ptr(parent), _ptr(port), nrows, _ptr(rows),
                                           _ptr(dsts), _ptr(last), n, _ptr(off), _ptr(sw),
                                           _ptr(hp), 0))
        return off, sw, hp

    def ecmp_counts(self, dist):
        """Shortest-route counts uint64 [D, V] from dist rows (saturating)."""
        dist = np.ascontiguousarray(dist, np.uint16)
        paths = np.empty(dist.shape, np.uint64)
        _check(self._lib.sdnr_ecmp_counts(self._h, _ptr(dist), int(dist.shape[0]), _ptr(paths), 0))
        return paths

    def ecmp_counts_device(self, dist_ptr, ndst, paths_ptr, timing=False):
        flags = DEVICE_PTRS | (TIMING if timing else 0)
        _check(self._lib.sdnr_ecmp_counts(self._h, ctypes.c_void_p(dist_ptr), int(ndst),
                                          ctypes.c_void_p(paths_ptr), flags))

    def ecmp_routes(self, dist, paths, rows, srcs, ranks, max_len):
        """Vertex sequences int32 [n, max_len] (-1 padded) of the ranks[k]-th
        lexicographic shortest route from srcs[k] in row rows[k]."""
        dist = np.ascontiguousarray(dist, np.uint16)
        paths = np.ascontiguousarray(paths, np.uint64)
        rows = np.ascontiguousarray(rows, np.int32)
        srcs = np.ascontiguousarray(srcs, np.int32)
        ranks = np.ascontiguousarray(ranks, np.uint64)
        n = int(rows.shape[0])
        out = np.empty((n, int(max_len)), np.int32)
        _check(self._lib.sdnr_ecmp_routes(self._h, _ptr(dist), _ptr(paths), int(dist.shape[0]),
                                          _ptr(rows), _ptr(srcs), _ptr(ranks), n, int(max_len),
                                          _ptr(out), 0))
        return out

    def ecmp_routes_device(self, dist_ptr, paths_ptr, ndst, rows_ptr, srcs_ptr, ranks_ptr,
                           nroutes, max_len, out_ptr):
        _check(self._lib.sdnr_ecmp_routes(self._h, ctypes.c_void_p(dist_ptr),
                                          ctypes.c_void_p(paths_ptr), int(ndst),
                                          ctypes.c_void_p(rows_ptr), ctypes.c_void_p(srcs_ptr),
                                          ctypes.c_void_p(ranks_ptr), int(nroutes), int(max_len),
                                          ctypes.c_void_p(out_ptr), DEVICE_PTRS))

    def route_offsets_device(self, hops_ptr, rows_ptr, dsts_ptr, npairs, off_ptr, nrows=0):
        _check(self._lib.sdnr_route_offsets(self._h, ctypes.c_void_p(hops_ptr), int(nrows),
                                            ctypes.c_void_p(rows_ptr), ctypes.c_void_p(dsts_ptr),
                                            int(npairs), ctypes.c_void_p(off_ptr), DEVICE_PTRS))

    def expand_routes_device(self, parent_ptr, port_ptr, nrows, rows_ptr, dsts_ptr, last_ptr,
                             npairs, off_ptr, sw_ptr, hp_ptr, timing=False, same_tables=False):
        flags = DEVICE_PTRS | (TIMING if timing else 0) | (SAME_TABLES if same_tables else 0)
        _check(self._lib.sdnr_route_expand(self._h, ctypes.c_void_p(parent_ptr),
                                           ctypes.c_void_p(port_ptr), int(nrows),
                                           ctypes.c_void_p(rows_ptr),
                                           ctypes.c_void_p(dsts_ptr), ctypes.c_void_p(last_ptr),
                                           int(npairs), ctypes.c_void_p(off_ptr),
                                           ctypes.c_void_p(sw_ptr), ctypes.c_void_p(hp_ptr), flags))

    def expand_routes_packed_device(self, parent_ptr, port_ptr, nrows, rows_ptr, dsts_ptr,
                                    last_ptr, npairs, off_ptr, ent_ptr, timing=False,
                                    same_tables=False):
        """Flow entries as one u32 each, switch | port << 16
        (sdnr_route_expand_packed, device pointers).  same_tables: the
        parent / port tables of the previous expansion on this context
        (SDNR_SAME_TABLES: its walk tables are reused)."""
        flags = DEVICE_PTRS | (TIMING if timing else 0) | (SAME_TABLES if same_tables else 0)
        _check(self._lib.sdnr_route_expand_packed(
            self._h, ctypes.c_void_p(parent_ptr), ctypes.c_void_p(port_ptr), int(nrows),
            ctypes.c_void_p(rows_ptr), ctypes.c_void_p(dsts_ptr), ctypes.c_void_p(last_ptr),
            int(npairs), ctypes.c_void_p(off_ptr), ctypes.c_void_p(ent_ptr), flags))

    def edge_ports(self, ends, ports):
        """bool [n_ports]: ports (uint64 keys) that are no link end (``ends``:
        sorted uint64 keys), see sdnr_edge_ports."""
        ends = np.ascontiguousarray(ends, np.uint64)
        ports = np.ascontiguousarray(ports, np.uint64)
        out = np.empty(ports.shape[0], np.uint8)
        _check(self._lib.sdnr_edge_ports(self._h, _ptr(ends), int(ends.shape[0]), _ptr(ports),
                                         int(ports.shape[0]), _ptr(out), 0))
        return out.astype(bool)

    def dfs_rows_affected_device(self, tree_ptr, depth_ptr, layout, depth_bytes, nrows,
                                 row_src_ptr, links_ptr, nremoved, nadded, affected_ptr,
                                 timing=False):
        """uint8 verdicts: which [nrows][V] tree rows the link changes alter
        (sdnr_dfs_rows_affected, device pointers, asynchronous)."""
        flags = DEVICE_PTRS | (TIMING if timing else 0)
        _check(self._lib.sdnr_dfs_rows_affected(
            self._h, ctypes.c_void_p(tree_ptr), ctypes.c_void_p(depth_ptr), int(layout),
            int(depth_bytes), int(nrows), ctypes.c_void_p(row_src_ptr),
            _p(links_ptr), int(nremoved), int(nadded),
            ctypes.c_void_p(affected_ptr), flags))

    def link_loads_device(self, tree_ptr, layout, nrows, pair_off_ptr, dsts_ptr, weight_ptr,
                          load_ptr, to_root=False, timing=False):
        """Add the per-link loads of a demand routed over [nrows][V] tree rows
        into ``load`` (u64 [E], CSR edge order; the caller zeroes it):
        sdnr_link_loads, device pointers, asynchronous.  ``weight_ptr`` 0:
        every pair weighs 1; ``to_root``: next-hop rows (SDNR_LOADS_TO_ROOT)."""
        flags = DEVICE_PTRS | (TIMING if timing else 0) | (LOADS_TO_ROOT if to_root else 0)
        _check(self._lib.sdnr_link_loads(
            self._h, _p(tree_ptr), int(layout), int(nrows), _p(pair_off_ptr), _p(dsts_ptr),
            _p(weight_ptr), _p(load_ptr), flags))

    def multicast_trees_device(self, tree_ptr, layout, nrows, ngroups, root_ptr, mem_off_ptr,
                               mem_row_ptr, mem_vertex_ptr, weight_ptr=0, reached_ptr=0,
                               ent_cnt_ptr=0, ent_off_ptr=0, ent_edge_ptr=0, load_ptr=0,
                               to_root=False, timing=False):
        """Multicast trees of ``ngroups`` groups over [nrows][V] tree rows
        (``to_root``: next-hop rows, SDNR_MCAST_TO_ROOT): sdnr_multicast_trees,
        device pointers, asynchronous.  A count call gives ``ent_cnt_ptr``
        (int64 [ngroups]), a fill call ``ent_off_ptr`` (its exclusive prefix)
        and ``ent_edge_ptr`` (int32 edge ids); ``load_ptr`` (u64 [E]) is ADDED
        into by the call that gets it, ``weight_ptr`` 0: every group weighs 1;
        ``reached_ptr``: u8 per member.  Pointers that are 0 are left out."""
        flags = DEVICE_PTRS | (TIMING if timing else 0) | (MCAST_TO_ROOT if to_root else 0)
        p = [_p(x) for x in (root_ptr, mem_off_ptr, mem_row_ptr, mem_vertex_ptr, weight_ptr,
                             reached_ptr, ent_cnt_ptr, ent_off_ptr, ent_edge_ptr, load_ptr)]
        _check(self._lib.sdnr_multicast_trees(
            self._h, _p(tree_ptr), int(layout), int(nrows), int(ngroups), *(p + [flags])))

    def ecmp_link_loads_device(self, dist_ptr, nrows, pair_off_ptr, srcs_ptr, weight_ptr,
                               load_ptr, hop=False, timing=False):
        """Add the per-link loads of a demand split over every shortest route
        of [nrows][V] u16 distance rows into ``load`` (f64 [E], CSR edge
        order; the caller zeroes it): sdnr_ecmp_link_loads, device pointers,
        asynchronous.  ``weight_ptr`` 0: every pair weighs 1; ``hop``: split
        evenly per switch (SDNR_LOADS_SPLIT_HOP) instead of per route."""
        flags = DEVICE_PTRS | (TIMING if timing else 0) | (LOADS_SPLIT_HOP if hop else 0)
        _check(self._lib.sdnr_ecmp_link_loads(
            self._h, _p(dist_ptr), int(nrows), _p(pair_off_ptr), _p(srcs_ptr), _p(weight_ptr),
            _p(load_ptr), flags))

    def cost_ecmp_link_loads_device(self, pcost_ptr, nrows, pair_off_ptr, srcs_ptr, weight_ptr,
                                    load_ptr, hop=False, timing=False):
        """Add the per-link loads of a demand split over every least-cost
        route of [nrows][V] u32 pcost rows (sdnr_cost_tables', under the costs
        in force) into ``load`` (f64 [E], CSR edge order; the caller zeroes
        it): sdnr_cost_ecmp_link_loads, device pointers, asynchronous.
        ``weight_ptr`` 0: every pair weighs 1; ``hop``: split evenly per
        switch (SDNR_LOADS_SPLIT_HOP) instead of per route."""
        flags = DEVICE_PTRS | (TIMING if timing else 0) | (LOADS_SPLIT_HOP if hop else 0)
        _check(self._lib.sdnr_cost_ecmp_link_loads(
            self._h, _p(pcost_ptr), int(nrows), _p(pair_off_ptr), _p(srcs_ptr), _p(weight_ptr),
            _p(load_ptr), flags))

    def failure_ecmp_link_loads_device(self, dst_ptr, nrows, pair_off_ptr, srcs_ptr, weight_ptr,
                                       nscen, scen_off_ptr, scen_edges_ptr, load_ptr, lost_ptr=0,
                                       routed_ptr=0, hop=False, timing=False):
        """Add the ECMP-over-least-cost link loads of a demand once per failure
        scenario into ``load`` (f64 [nscen][E]; the caller zeroes it), the
        scenario's links (CSR edge indices ``scen_edges[scen_off[k] ..
        scen_off[k+1])``, ascending) masked out; ``lost`` (f64 [nscen], added
        into) and ``routed`` (u8 [nscen][npairs], written) may be 0:
        sdnr_failure_ecmp_link_loads, device pointers, asynchronous.  Row r
        routes toward dense switch ``dst[r]`` under the costs in force (none
        uploaded: every link costs 1).  ``weight_ptr`` 0: every pair weighs 1;
        ``hop``: split evenly per switch (SDNR_LOADS_SPLIT_HOP)."""
        flags = DEVICE_PTRS | (TIMING if timing else 0) | (LOADS_SPLIT_HOP if hop else 0)
        _check(self._lib.sdnr_failure_ecmp_link_loads(
            self._h, _p(dst_ptr), int(nrows), _p(pair_off_ptr), _p(srcs_ptr), _p(weight_ptr),
            int(nscen), _p(scen_off_ptr), _p(scen_edges_ptr), _p(load_ptr), _p(lost_ptr),
            _p(routed_ptr), flags))

    def whatif_ecmp_link_loads_device(self, dst_ptr, nrows, pair_off_ptr, srcs_ptr, weight_ptr,
                                      nscen, scen_off_ptr, scen_edges_ptr, scen_costs_ptr,
                                      load_ptr, lost_ptr=0, routed_ptr=0, capacity_ptr=0,
                                      peak_ptr=0, peak_edge_ptr=0, hop=False, timing=False):
        """Add the ECMP-over-least-cost link loads of a demand once per cost
        scenario into ``load`` (f64 [nscen][E]; the caller zeroes it), the
        scenario's overrides (CSR edge indices ``scen_edges[scen_off[k] ..
        scen_off[k+1])``, strictly ascending, with the costs ``scen_costs``
        beside them, COST_INF: the link is down) in force; ``lost`` and
        ``routed`` as in ``failure_ecmp_link_loads_device``.  ``peak`` (f64
        [nscen]) and ``peak_edge`` (int32 [nscen]), both or neither, are
        written: the largest ``load[k][e] / capacity[e]`` (``capacity_ptr`` 0:
        1.0 per link) and the first link that attains it:
        sdnr_whatif_ecmp_link_loads, device pointers, asynchronous."""
        flags = DEVICE_PTRS | (TIMING if timing else 0) | (LOADS_SPLIT_HOP if hop else 0)
        _check(self._lib.sdnr_whatif_ecmp_link_loads(
            self._h, _p(dst_ptr), int(nrows), _p(pair_off_ptr), _p(srcs_ptr), _p(weight_ptr),
            int(nscen), _p(scen_off_ptr), _p(scen_edges_ptr), _p(scen_costs_ptr), _p(load_ptr),
            _p(lost_ptr), _p(routed_ptr), _p(capacity_ptr), _p(peak_ptr), _p(peak_edge_ptr), flags))

    def frr_link_loads_device(self, dst_ptr, nh_ptr, backup_ptr, nrows, pair_off_ptr, srcs_ptr,
                              weight_ptr, nscen, scen_off_ptr, scen_edges_ptr, load_ptr,
                              stat_ptr=0, status_ptr=0, peak_ptr=0, peak_edge_ptr=0, timing=False):
        """Add the link loads of a demand while the backup next hops forward,
        once per failure scenario, into ``load`` (u64 [nscen][E]; the caller
        zeroes it): row r forwards toward ``dst[r]`` over ``nh`` (int32
        [nrows][V]) and, where the scenario took the primary link, over
        ``backup`` (the same shape); scenarios as in
        ``failure_ecmp_link_loads_device``.  ``stat`` (u64 [nscen][4], added
        into: the weight repaired, dropped, looped, without a base route),
        ``status`` (u8 [nscen][npairs], written: 0 no base route, 1 primary,
        2 repaired, 3 dropped, 4 looped) and ``peak`` / ``peak_edge`` (u64 /
        int32 [nscen], written, both or neither) may be 0:
        sdnr_frr_link_loads, device pointers, asynchronous."""
        flags = DEVICE_PTRS | (TIMING if timing else 0)
        _check(self._lib.sdnr_frr_link_loads(
            self._h, _p(dst_ptr), _p(nh_ptr), _p(backup_ptr), int(nrows), _p(pair_off_ptr),
            _p(srcs_ptr), _p(weight_ptr), int(nscen), _p(scen_off_ptr), _p(scen_edges_ptr),
            _p(load_ptr), _p(stat_ptr), _p(status_ptr), _p(peak_ptr), _p(peak_edge_ptr), flags))

    def lfa_tables_device(self, pcost_all_ptr, dst_ptr, ndst, backup_ptr, backup_port_ptr,
                          kind_ptr, counts_ptr=0, link_only=False, timing=False):
        """Loop-free alternate next hops of ``ndst`` destinations
        (sdnr_lfa_tables, device pointers, asynchronous): ``pcost_all`` u32
        [V][V], row v = the least costs toward v under the costs in force (none
        uploaded: every link costs 1); written: ``backup``, ``backup_port``
        int32 [ndst][V], ``kind`` u8 [ndst][V] (1 = a backup exists, 2 =
        downstream, 4 = node-protecting) and, unless 0, ``counts`` u32
        [ndst][4] (primaries, backups, node-protecting, downstream).
        ``link_only``: SDNR_LFA_LINK_ONLY."""
        flags = DEVICE_PTRS | (TIMING if timing else 0) | (LFA_LINK_ONLY if link_only else 0)
        _check(self._lib.sdnr_lfa_tables(
            self._h, _p(pcost_all_ptr), _p(dst_ptr), int(ndst), _p(backup_ptr), _p(backup_port_ptr),
            _p(kind_ptr), _p(counts_ptr), flags))

    def remote_lfa_device(self, pcost_all_ptr, verts_ptr, nverts, pq_ptr, via_ptr, via_port_ptr,
                          tunnel_cost_ptr, kind_ptr, counts_ptr=0, timing=False):
        """Remote loop-free alternates of the out-links of ``nverts`` source
        vertices (sdnr_remote_lfa, device pointers, asynchronous):
        ``pcost_all`` u32 [V][V] as in ``lfa_tables_device``; ``verts`` int32
        [nverts] or 0 (0 .. nverts - 1); written, in CSR edge order and only
        at the out-links of the listed vertices: ``pq``, ``via``, ``via_port``
        int32 [E], ``tunnel_cost`` u64 [E], ``kind`` u8 [E] (1 = a repair
        exists, 2 = the PQ node is in the source's own P-space, 4 = it is the
        neighbour itself) and, unless 0, ``counts`` u32 [nverts][4] (links
        that are no self-loops, repaired, kind & 2, kind & 4)."""
        flags = DEVICE_PTRS | (TIMING if timing else 0)
        _check(self._lib.sdnr_remote_lfa(
            self._h, _p(pcost_all_ptr), _p(verts_ptr), int(nverts), _p(pq_ptr), _p(via_ptr),
            _p(via_port_ptr), _p(tunnel_cost_ptr), _p(kind_ptr), _p(counts_ptr), flags))

    def apsp(self):
        dist = np.empty((self.V, self.V), np.uint16)
        _check(self._lib.sdnr_apsp(self._h, _ptr(dist), 0))
        return dist

    # -- device-pointer (asynchronous) calls --------------------------
    def dfs_tables_device(self, src_ptr, nsrc, parent_ptr, port_ptr, hops_ptr=0,
                          timing=False):
        flags = DEVICE_PTRS | (TIMING if timing else 0)
        _check(self._lib.sdnr_dfs_tables(
            self._h, ctypes.c_void_p(src_ptr), int(nsrc), ctypes.c_void_p(parent_ptr),
            ctypes.c_void_p(port_ptr), _p(hops_ptr),
            flags))

    def dfs_tables_packed_device(self, src_ptr, nsrc, tree_ptr, timing=False):
        flags = DEVICE_PTRS | (TIMING if timing else 0)
        _check(self._lib.sdnr_dfs_tables_packed(self._h, ctypes.c_void_p(src_ptr), int(nsrc),
                                                ctypes.c_void_p(tree_ptr), flags))

    def dfs_tables_slots_device(self, src_ptr, nsrc, tree_ptr, timing=False):
        flags = DEVICE_PTRS | (TIMING if timing else 0)
        _check(self._lib.sdnr_dfs_tables_slots(self._h, ctypes.c_void_p(src_ptr), int(nsrc),
                                               ctypes.c_void_p(tree_ptr), flags))

    def dfs_tables_tree_device(self, src_ptr, nsrc, tree_ptr, depth_ptr, layout, depth_bytes,
                               timing=False):
        """Trees in a 4-byte layout (TREE_PORT16 / TREE_SLOT) plus depths
        (u16 or int32, ``depth_bytes`` 2 / 4; depth_ptr 0: none) straight
        from the DFS kernels (sdnr_dfs_tables_tree)."""
        flags = DEVICE_PTRS | (TIMING if timing else 0)
        _check(self._lib.sdnr_dfs_tables_tree(
            self._h, ctypes.c_void_p(src_ptr), int(nsrc), ctypes.c_void_p(tree_ptr),
            _p(depth_ptr), int(layout), int(depth_bytes),
            flags))

    def dfs_tables_tree(self, srcs, layout, depth_bytes=2):
        """Host-buffer form of dfs_tables_tree_device: (tree uint32 [S, V],
        depth uint16 / int32 [S, V])."""
        srcs = np.ascontiguousarray(srcs, np.int32)
        S, V = int(srcs.shape[0]), self.V
        tree = np.empty((S, V), np.uint32)
        depth = np.empty((S, V), np.uint16 if depth_bytes == 2 else np.int32)
        _check(self._lib.sdnr_dfs_tables_tree(self._h, _ptr(srcs), S, _ptr(tree), _ptr(depth),
                                              int(layout), int(depth_bytes), 0))
        return tree, depth

    def tree_pack_device(self, parent_ptr, port_ptr, n, tree_ptr, layout):
        """int32 parent/port tables (device) -> 4-byte trees (sdnr_tree_pack)."""
        _check(self._lib.sdnr_tree_pack(self._h, ctypes.c_void_p(parent_ptr),
                                        _p(port_ptr), int(n), ctypes.c_void_p(tree_ptr),
                                        int(layout), DEVICE_PTRS))

    def shortest_tables_device(self, dst_ptr, ndst, dist_ptr, nh_ptr=0, nh_port_ptr=0,
                               timing=False):
        flags = DEVICE_PTRS | (TIMING if timing else 0)
        _check(self._lib.sdnr_shortest_tables(
            self._h, ctypes.c_void_p(dst_ptr), int(ndst), ctypes.c_void_p(dist_ptr),
            _p(nh_ptr), _p(nh_port_ptr), flags))

    def cost_tables_device(self, dst_ptr, ndst, pcost_ptr, nh_ptr=0, nh_port_ptr=0,
                           timing=False):
        """sdnr_cost_tables over device buffers (pcost u32, nh / nh_port int32
        [ndst][V]; both next-hop pointers or neither), asynchronous."""
        flags = DEVICE_PTRS | (TIMING if timing else 0)
        _check(self._lib.sdnr_cost_tables(
            self._h, ctypes.c_void_p(dst_ptr), int(ndst), ctypes.c_void_p(pcost_ptr),
            _p(nh_ptr), _p(nh_port_ptr), flags))

    def widest_tables_device(self, pcost_ptr, util_ptr, dst_ptr, ndst, bott_ptr, nh_ptr=0,
                             nh_port_ptr=0, timing=False):
        """sdnr_widest_tables over device buffers (pcost, bott u32, nh /
        nh_port int32 [ndst][V]; util u32 [E]; both next-hop pointers or
        neither), asynchronous."""
        flags = DEVICE_PTRS | (TIMING if timing else 0)
        _check(self._lib.sdnr_widest_tables(
            self._h, _p(pcost_ptr), _p(util_ptr), _p(dst_ptr), int(ndst), _p(bott_ptr), _p(nh_ptr),
            _p(nh_port_ptr), flags))

    def fair_rates_device(self, tree_ptr, layout, nrows, pair_off_ptr, verts_ptr, mult_ptr,
                          extra_ptr, cap_ptr, nextra, rate_ptr, bott_ptr, round_ptr, level_ptr,
                          max_rounds, used_ptr, to_root=False, timing=False):
        """Max-min fair rates of flows routed over [nrows][V] tree rows
        (sdnr_fair_rates, device pointers): writes rate (f64), bott and round
        (i32) per flow, level (f64 [max_rounds]) and used (f64 [E + nextra]),
        and returns the number of rounds.  ``mult_ptr`` 0: every flow counts
        once; ``extra_ptr`` 0: no extra constraints; ``to_root``: next-hop
        rows (SDNR_LOADS_TO_ROOT).  Waits for the rounds; errors of the rows
        surface in ``synchronize``."""
        flags = DEVICE_PTRS | (TIMING if timing else 0) | (LOADS_TO_ROOT if to_root else 0)
        n = ctypes.c_int32()
        _check(self._lib.sdnr_fair_rates(
            self._h, _p(tree_ptr), int(layout), int(nrows), _p(pair_off_ptr), _p(verts_ptr),
            _p(mult_ptr), _p(extra_ptr), _p(cap_ptr), int(nextra), _p(rate_ptr), _p(bott_ptr),
            _p(round_ptr), _p(level_ptr), int(max_rounds), _p(used_ptr), ctypes.byref(n), flags))
        return n.value

    def fair_times_device(self, tree_ptr, layout, nrows, pair_off_ptr, verts_ptr, mult_ptr,
                          bytes_ptr, extra_ptr, cap_ptr, nextra, time_ptr, epoch_ptr, rate0_ptr,
                          remaining_ptr, epoch_time_ptr, epoch_rounds_ptr, max_epochs,
                          carried_ptr, to_root=False, timing=False):
        """Max-min fair completion times of flows routed over [nrows][V] tree
        rows (sdnr_fair_times, device pointers): writes time, rate0 and
        remaining (f64) and epoch (i32) per flow, epoch_time (f64) and
        epoch_rounds (i32) [max_epochs] and carried (f64 [E + nextra]), and
        returns the number of epochs.  ``bytes_ptr``: f64 per flow; the other
        arguments as in ``fair_rates_device``.  Waits for the epochs; errors
        of the rows surface in ``synchronize``."""
        flags = DEVICE_PTRS | (TIMING if timing else 0) | (LOADS_TO_ROOT if to_root else 0)
        n = ctypes.c_int32()
        _check(self._lib.sdnr_fair_times(
            self._h, _p(tree_ptr), int(layout), int(nrows), _p(pair_off_ptr), _p(verts_ptr),
            _p(mult_ptr), _p(bytes_ptr), _p(extra_ptr), _p(cap_ptr), int(nextra), _p(time_ptr),
            _p(epoch_ptr), _p(rate0_ptr), _p(remaining_ptr), _p(epoch_time_ptr),
            _p(epoch_rounds_ptr), int(max_epochs), _p(carried_ptr), ctypes.byref(n), flags))
        return n.value

    def ecmp_fair_rates_device(self, pcost_ptr, nrows, pair_off_ptr, srcs_ptr, mult_ptr,
                               extra_ptr, cap_ptr, nextra, rate_ptr, bott_ptr, round_ptr,
                               level_ptr, max_rounds, used_ptr, hop=False, timing=False):
        """Max-min fair rates of flows split over every least-cost route of
        [nrows][V] u32 pcost rows under the costs in force (none uploaded:
        every link costs 1; sdnr_ecmp_fair_rates, device pointers): writes
        rate (f64), bott and round (i32) per flow, level (f64 [max_rounds])
        and used (f64 [E + nextra]), and returns the number of rounds.
        ``mult_ptr`` 0: every flow counts once; ``extra_ptr`` 0: no extra
        constraints; ``hop``: SDNR_LOADS_SPLIT_HOP.  Waits for the rounds;
        errors of the rows surface in ``synchronize``."""
        flags = DEVICE_PTRS | (TIMING if timing else 0) | (LOADS_SPLIT_HOP if hop else 0)
        n = ctypes.c_int32()
        _check(self._lib.sdnr_ecmp_fair_rates(
            self._h, _p(pcost_ptr), int(nrows), _p(pair_off_ptr), _p(srcs_ptr), _p(mult_ptr),
            _p(extra_ptr), _p(cap_ptr), int(nextra), _p(rate_ptr), _p(bott_ptr), _p(round_ptr),
            _p(level_ptr), int(max_rounds), _p(used_ptr), ctypes.byref(n), flags))
        return n.value

    def ecmp_fair_times_device(self, pcost_ptr, nrows, pair_off_ptr, srcs_ptr, mult_ptr,
                               bytes_ptr, extra_ptr, cap_ptr, nextra, time_ptr, epoch_ptr,
                               rate0_ptr, remaining_ptr, epoch_time_ptr, epoch_rounds_ptr,
                               max_epochs, carried_ptr, hop=False, timing=False):
        """Max-min fair completion times of flows split over every least-cost
        route of [nrows][V] u32 pcost rows (sdnr_ecmp_fair_times, device
        pointers): the outputs of ``fair_times_device`` over the flows of
        ``ecmp_fair_rates_device``, and returns the number of epochs.
        ``bytes_ptr``: f64 per flow; ``hop``: SDNR_LOADS_SPLIT_HOP.  Waits for
        the epochs; errors of the rows surface in ``synchronize``."""
        flags = DEVICE_PTRS | (TIMING if timing else 0) | (LOADS_SPLIT_HOP if hop else 0)
        n = ctypes.c_int32()
        _check(self._lib.sdnr_ecmp_fair_times(
            self._h, _p(pcost_ptr), int(nrows), _p(pair_off_ptr), _p(srcs_ptr), _p(mult_ptr),
            _p(bytes_ptr), _p(extra_ptr), _p(cap_ptr), int(nextra), _p(time_ptr), _p(epoch_ptr),
            _p(rate0_ptr), _p(remaining_ptr), _p(epoch_time_ptr), _p(epoch_rounds_ptr),
            int(max_epochs), _p(carried_ptr), ctypes.byref(n), flags))
        return n.value

    def apsp_device(self, dist_ptr, timing=False):
        flags = DEVICE_PTRS | (TIMING if timing else 0)
        _check(self._lib.sdnr_apsp(self._h, ctypes.c_void_p(dist_ptr), flags))

    def last_kernel(self):
        return self._lib.sdnr_last_kernel(self._h).decode()

    def last_launches(self):
        n = ctypes.c_int32()
        _check(self._lib.sdnr_last_launches(self._h, ctypes.byref(n)))
        return n.value

    def last_grid(self):
        """Workgroups of the last row-persistent launch (sdnr_last_grid): with
        more rows, batches, items or groups than this a workgroup took more
        than one."""
        n = ctypes.c_int64()
        _check(self._lib.sdnr_last_grid(self._h, ctypes.byref(n)))
        return n.value

    def twin_reps(self):
        """rep[V]: the smallest vertex of each vertex's twin class
        (sdnr_graph_twin_reps)."""
        rep = np.empty(max(self.V, 0), np.int32)
        _check(self._lib.sdnr_graph_twin_reps(self._h, _ptr(rep)))
        return rep

    def last_frr_items(self):
        """(Scenario, row) items the last ``frr_link_loads_device`` call
        recomputed -- the affected ones (sdnr_last_frr_items; waits)."""
        n = ctypes.c_int64(0)
        _check(self._lib.sdnr_last_frr_items(self._h, ctypes.byref(n)))
        return int(n.value)

    def last_dfs_searched(self):
        """Sources the last DFS table call searched: fewer than the batch when
        it folded twin classes (sdnr_last_dfs_searched)."""
        n = ctypes.c_int32()
        _check(self._lib.sdnr_last_dfs_searched(self._h, ctypes.byref(n)))
        return n.value

    def last_dfs_form(self):
        """"full" or "low": the form of the search kernel in the last DFS table
        call (sdnr_last_dfs_form; low: a folded call after one that left few
        live searches)."""
        n = ctypes.c_int32()
        _check(self._lib.sdnr_last_dfs_form(self._h, ctypes.byref(n)))
        return "low" if n.value else "full"

    def last_dfs_quotient(self):
        """1 when the search kernel of the last DFS table call ran on the
        twin-class quotient, else 0 (sdnr_last_dfs_quotient)."""
        n = ctypes.c_int32()
        _check(self._lib.sdnr_last_dfs_quotient(self._h, ctypes.byref(n)))
        return n.value

    def last_sweeps(self):
        """Bellman-Ford sweeps of the last APSP call (sdnr_last_sweeps)."""
        n = ctypes.c_int32()
        _check(self._lib.sdnr_last_sweeps(self._h, ctypes.byref(n)))
        return n.value

    def last_kernel_ms(self):
        ms = ctypes.c_float()
        _check(self._lib.sdnr_last_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value
