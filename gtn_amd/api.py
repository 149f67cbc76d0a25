"""Host-side mirror of the reference's Python interface over the C ABI.

Names, argument meaning and error behaviour follow bindings/python/gtn
(`_graph.cpp:20-110`, `_functions.cpp:18-200`, `_autograd.cpp`, `_creations.cpp`,
`_utils.cpp`): `Graph.add_node/add_arc/...`, `compose`, `intersect`,
`forward_score`, `viterbi_score`, `viterbi_path`, `negate/add/subtract`,
`backward`, `linear_graph`, `scalar_graph`, `equal`, `isomorphic`.  As in the
reference binding every graph function also accepts lists of graphs
(`_functions.cpp:84-135`); here a list runs as ONE batched device launch per
kernel (`gtnx_*_n`) instead of `parallelMap` over CPU threads.

`make_api(lib)` binds this interface to one loaded library, so the tests can
hold the product (libgtn_amd.so) and the reference shim (libgtn_ref.so) side by
side.
"""
import ctypes as C
import math
import types

import numpy as np

from . import _capi

_EXC = {
    _capi.INVALID_ARGUMENT: ValueError,   # pybind11 maps std::invalid_argument -> ValueError
    _capi.LOGIC_ERROR: RuntimeError,      # std::logic_error -> RuntimeError
    _capi.RUNTIME_ERROR: RuntimeError,
    _capi.OUT_OF_RANGE: IndexError,
    _capi.DEVICE_ERROR: RuntimeError,
}


class GtnError(RuntimeError):
    pass


def _is_seq(x):
    return isinstance(x, (list, tuple))


def make_api(lib):
    ns = types.SimpleNamespace()
    ns.lib = lib
    ns.epsilon = -1

    def check(status):
        if status != 0:
            msg = lib.gtnx_last_error().decode("utf-8", "replace")
            raise _EXC.get(status, GtnError)(msg)

    ns.check = check

    def _harr(graphs):
        arr = (C.c_void_p * len(graphs))(*[g._h for g in graphs])
        return arr

    def _wrap_many(arr, n):
        return [Graph._from_handle(arr[i]) for i in range(n)]

    def _as_dev_ptr(x):
        """torch ROCm tensor / object with data_ptr() / int address -> int"""
        if hasattr(x, "data_ptr"):
            return int(x.data_ptr())
        return int(x)

    def _opt_ptr(x):
        """_as_dev_ptr of an argument that may be None"""
        return _as_dev_ptr(x) if x is not None else None

    def _row_tensors(who, names, tensors, n, row_stride, width_name):
        """the one row stride of the int32 [B, width] outputs among `tensors` (None and device addresses are passed
        over: those go by `row_stride`)"""
        stride = row_stride
        for t in tensors:
            if t is None or not hasattr(t, "data_ptr"):
                continue
            if t.element_size() != 4 or t.dim() != 2 or t.shape[0] < n or (t.shape[1] > 1 and t.stride(1) != 1):
                raise ValueError(f"{who}: outputs must be int32 tensors [B, {width_name}] with contiguous rows")
            if stride is not None and t.stride(0) != stride:
                raise ValueError(f"{who}: {names} must have the same row stride")
            stride = t.stride(0)
        if stride is None:
            raise ValueError(f"{who}: a device address needs row_stride")
        return int(stride)

    def _frames_arg(who, frames, n):
        """(host int32 array [n] or None, its address or None) of per-element frame counts; the caller keeps the array"""
        if frames is None:
            return None, None
        fr = np.ascontiguousarray(frames, dtype=np.int32)
        if fr.shape != (n,):
            raise ValueError(f"{who}: one frame count per element")
        return fr, fr.ctypes.data

    def _stats2(cfn):
        """the two counters of a gtnx_*_stats getter"""
        a, b = C.c_int64(0), C.c_int64(0)
        check(cfn(C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    class Graph:
        """gtn.Graph (bindings/python/gtn/_graph.cpp:23-108)."""

        __slots__ = ("_h", "__weakref__")

        def __init__(self, calc_grad=True):
            h = C.c_void_p()
            check(lib.gtnx_graph_create(1 if calc_grad else 0, C.byref(h)))
            self._h = h.value

        @classmethod
        def _from_handle(cls, h):
            g = object.__new__(cls)
            g._h = h
            return g

        def __del__(self):
            h = getattr(self, "_h", None)
            if h:
                try:
                    lib.gtnx_graph_destroy(h)
                except Exception:
                    pass
                self._h = None

        # -- construction ---------------------------------------------------
        def add_node(self, start=False, accept=False):
            i = C.c_int()
            check(lib.gtnx_graph_add_node(self._h, int(bool(start)), int(bool(accept)), C.byref(i)))
            return i.value

        def add_arc(self, src_node, dst_node, ilabel=None, olabel=None, weight=0.0, label=None):
            """add_arc(src_node, dst_node, label) / add_arc(src_node, dst_node, ilabel, olabel, weight=0.0)
            (the binding's two overloads, _graph.cpp:30-43)"""
            if label is not None:
                if ilabel is not None or olabel is not None:
                    raise TypeError("add_arc: give either label or ilabel / olabel")
                ilabel = label
            if ilabel is None:
                raise TypeError("add_arc: missing label")
            if olabel is None:
                olabel = ilabel
            i = C.c_int()
            check(lib.gtnx_graph_add_arc(self._h, int(src_node), int(dst_node), int(ilabel),
                                         int(olabel), float(weight), C.byref(i)))
            return i.value

        def add_nodes(self, start, accept):
            """bulk add_node (extension; same order as successive calls)"""
            s = np.ascontiguousarray(start, dtype=np.uint8)
            a = np.ascontiguousarray(accept, dtype=np.uint8)
            assert s.shape == a.shape
            check(lib.gtnx_graph_add_nodes(self._h, s.size, s.ctypes.data, a.ctypes.data))

        def add_arcs(self, src, dst, ilabel, olabel=None, weight=None):
            """bulk add_arc (extension)"""
            src = np.ascontiguousarray(src, dtype=np.int32)
            dst = np.ascontiguousarray(dst, dtype=np.int32)
            il = np.ascontiguousarray(ilabel, dtype=np.int32)
            ol = il if olabel is None else np.ascontiguousarray(olabel, dtype=np.int32)
            w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float32)
            check(lib.gtnx_graph_add_arcs(self._h, src.size, src.ctypes.data, dst.ctypes.data,
                                          il.ctypes.data, ol.ctypes.data,
                                          None if w is None else w.ctypes.data))

        # -- counts -----------------------------------------------------------
        def _count(self, fn):
            v = C.c_int64()
            check(fn(self._h, C.byref(v)))
            return v.value

        def num_arcs(self):
            return self._count(lib.gtnx_graph_num_arcs)

        def num_nodes(self):
            return self._count(lib.gtnx_graph_num_nodes)

        def num_start(self):
            return self._count(lib.gtnx_graph_num_start)

        def num_accept(self):
            return self._count(lib.gtnx_graph_num_accept)

        def item(self):
            v = C.c_float()
            check(lib.gtnx_graph_item(self._h, C.byref(v)))
            return v.value

        # -- sorting ------------------------------------------------------------
        def arc_sort(self, olabel=False):
            check(lib.gtnx_graph_arc_sort(self._h, int(bool(olabel))))

        def mark_arc_sorted(self, olabel=False):
            check(lib.gtnx_graph_mark_arc_sorted(self._h, int(bool(olabel))))

        def ilabel_sorted(self):
            v = C.c_int()
            check(lib.gtnx_graph_ilabel_sorted(self._h, C.byref(v)))
            return bool(v.value)

        def olabel_sorted(self):
            v = C.c_int()
            check(lib.gtnx_graph_olabel_sorted(self._h, C.byref(v)))
            return bool(v.value)

        # -- weights ------------------------------------------------------------
        def weights(self):
            """address of the live host weight buffer (as the reference returns)"""
            p = _capi.c_f32_p()
            check(lib.gtnx_graph_weights(self._h, 1, C.byref(p)))
            return C.cast(p, C.c_void_p).value or 0

        def weights_to_numpy(self):
            out = np.empty(self.num_arcs(), dtype=np.float32)
            check(lib.gtnx_graph_get_weights(self._h, out.ctypes.data))
            return out

        def weights_to_list(self):
            return self.weights_to_numpy().tolist()

        def weights_device(self):
            """device address of the weight buffer (extension)"""
            p = C.c_void_p()
            check(lib.gtnx_graph_weights_device(self._h, C.byref(p)))
            return p.value or 0

        def set_weights(self, weights):
            """list / numpy array / host address (reference overloads), or a
            ROCm torch tensor, which is copied device-to-device."""
            if hasattr(weights, "is_cuda") and weights.is_cuda:
                if weights.numel() != self.num_arcs() or str(weights.dtype) != "torch.float32":
                    raise ValueError("set_weights: need numArcs float32 values")
                w = weights.contiguous()
                check(lib.gtnx_graph_set_weights_device(self._h, w.data_ptr()))
                return
            if hasattr(weights, "detach"):
                weights = weights.detach().cpu().numpy()
            if isinstance(weights, int):
                check(lib.gtnx_graph_set_weights(self._h, weights))
                return
            w = np.ascontiguousarray(weights, dtype=np.float32)
            if w.size != self.num_arcs():
                raise ValueError("set_weights: need numArcs values")
            check(lib.gtnx_graph_set_weights(self._h, w.ctypes.data))

        def set_weights_device(self, ptr):
            check(lib.gtnx_graph_set_weights_device(self._h, _as_dev_ptr(ptr)))

        def labels_to_list(self, ilabel=True):
            out = np.empty(self.num_arcs(), dtype=np.int32)
            check(lib.gtnx_graph_labels_to_array(self._h, out.ctypes.data, int(bool(ilabel))))
            return out.tolist()

        # -- grad ----------------------------------------------------------------
        @property
        def calc_grad(self):
            v = C.c_int()
            check(lib.gtnx_graph_calc_grad(self._h, C.byref(v)))
            return bool(v.value)

        @calc_grad.setter
        def calc_grad(self, value):
            check(lib.gtnx_graph_set_calc_grad(self._h, int(bool(value))))

        def is_grad_available(self):
            v = C.c_int()
            check(lib.gtnx_graph_is_grad_available(self._h, C.byref(v)))
            return bool(v.value)

        def grad(self):
            h = C.c_void_p()
            check(lib.gtnx_graph_grad(self._h, C.byref(h)))
            return Graph._from_handle(h.value)

        def zero_grad(self):
            check(lib.gtnx_graph_zero_grad(self._h))

        def add_grad(self, other):
            if isinstance(other, Graph):
                check(lib.gtnx_graph_add_grad_graph(self._h, other._h))
            else:
                v = np.ascontiguousarray(other, dtype=np.float32)
                check(lib.gtnx_graph_add_grad(self._h, v.ctypes.data, v.size))

        def id(self):
            v = C.c_size_t()
            check(lib.gtnx_graph_id(self._h, C.byref(v)))
            return v.value

        # -- structure inspection (C++ accessors, graph.h:330-414) -----------------
        def start(self):
            out = np.empty(self.num_start(), dtype=np.int32)
            check(lib.gtnx_graph_get_start(self._h, out.ctypes.data))
            return out.tolist()

        def accept(self):
            out = np.empty(self.num_accept(), dtype=np.int32)
            check(lib.gtnx_graph_get_accept(self._h, out.ctypes.data))
            return out.tolist()

        def is_start(self, n):
            v = C.c_int()
            check(lib.gtnx_graph_is_start(self._h, n, C.byref(v)))
            return bool(v.value)

        def is_accept(self, n):
            v = C.c_int()
            check(lib.gtnx_graph_is_accept(self._h, n, C.byref(v)))
            return bool(v.value)

        def make_accept(self, n):
            check(lib.gtnx_graph_make_accept(self._h, n))

        def out(self, n):
            c = C.c_int64()
            check(lib.gtnx_graph_num_out(self._h, n, C.byref(c)))
            out = np.empty(c.value, dtype=np.int32)
            check(lib.gtnx_graph_get_out(self._h, n, out.ctypes.data))
            return out.tolist()

        def in_(self, n):
            c = C.c_int64()
            check(lib.gtnx_graph_num_in(self._h, n, C.byref(c)))
            out = np.empty(c.value, dtype=np.int32)
            check(lib.gtnx_graph_get_in(self._h, n, out.ctypes.data))
            return out.tolist()

        def arcs(self):
            """(src, dst, ilabel, olabel, weight) numpy arrays in arc-id order"""
            A = self.num_arcs()
            s, d, i, o = (np.empty(A, dtype=np.int32) for _ in range(4))
            check(lib.gtnx_graph_get_arcs(self._h, s.ctypes.data, d.ctypes.data,
                                          i.ctypes.data, o.ctypes.data))
            return s, d, i, o, self.weights_to_numpy()

        def arc(self, a):
            s, d, i, o, w = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_float()
            check(lib.gtnx_graph_get_arc(self._h, a, C.byref(s), C.byref(d), C.byref(i),
                                         C.byref(o), C.byref(w)))
            return s.value, d.value, i.value, o.value, w.value

        def set_weight(self, a, w):
            check(lib.gtnx_graph_set_weight(self._h, a, float(w)))

        def copy(self):
            h = C.c_void_p()
            check(lib.gtnx_graph_copy(self._h, C.byref(h)))
            return Graph._from_handle(h.value)

        def deep_copy(self):
            h = C.c_void_p()
            check(lib.gtnx_graph_deep_copy(self._h, C.byref(h)))
            return Graph._from_handle(h.value)

        def __repr__(self):
            host = _host(required=False)
            if host is not None:  # operator<< of utils.h (what the binding prints)
                need = C.c_size_t()
                hcheck(host.gtnh_repr(self._h, None, 0, C.byref(need)))
                buf = C.create_string_buffer(need.value)
                hcheck(host.gtnh_repr(self._h, buf, need.value, None))
                return buf.value.decode()
            s, d, i, o, w = self.arcs()
            lines = [" ".join(map(str, self.start())), " ".join(map(str, self.accept()))]
            lines += [f"{a} {b} {c} {e} {f:g}" for a, b, c, e, f in zip(s, d, i, o, w)]
            return "\n".join(lines)

    ns.Graph = Graph

    # ---------------------------------------------------------------- host-side builders / formats
    # gtn_amd/hostops: C entry points over include/gtn's header-only clone / project / concat / closure /
    # union / remove / sample / randEquivalent / load / save / draw.  One copy sits next to (and is linked
    # against) each C-ABI library; RTLD_DEEPBIND keeps its gtnx_* calls on that library even when the
    # product and the reference shim are loaded side by side.
    _hostlib = []

    def _host(required=True):
        if not _hostlib:
            import os
            path = os.path.join(os.path.dirname(os.path.abspath(getattr(lib, "_path", ""))), "libgtn_hostops.so")
            h = None
            if os.path.exists(path):
                h = C.CDLL(path, mode=getattr(os, "RTLD_DEEPBIND", 0) | getattr(os, "RTLD_NOW", 2))
                vp, vpp, ip = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int)
                for name, args in {
                    "gtnh_clone": [vp, C.c_int, vpp], "gtnh_concat": [vpp, C.c_int, vpp], "gtnh_closure": [vp, vpp],
                    "gtnh_union": [vpp, C.c_int, vpp], "gtnh_remove": [vp, C.c_int, C.c_int, vpp],
                    "gtnh_sample": [vp, C.c_size_t, vpp],
                    "gtnh_rand_equivalent": [vp, vp, C.c_size_t, C.c_double, C.c_size_t, ip],
                    "gtnh_load": [C.c_char_p, vpp], "gtnh_save": [C.c_char_p, vp],
                    "gtnh_loadtxt": [C.c_char_p, vpp], "gtnh_savetxt": [C.c_char_p, vp],
                    "gtnh_write_dot": [vp, C.c_char_p, ip, C.POINTER(C.c_char_p), C.c_int, ip, C.POINTER(C.c_char_p),
                                       C.c_int],
                    "gtnh_repr": [vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)],
                }.items():
                    fn = getattr(h, name)
                    fn.argtypes = args
                    fn.restype = C.c_int
                h.gtnh_last_error.restype = C.c_char_p
            _hostlib.append(h)
        if _hostlib[0] is None and required:
            raise ImportError("gtn_amd: libgtn_hostops.so not found next to the C-ABI library "
                              "(python -c 'import __graft_entry__ as g; g.build()')")
        return _hostlib[0]

    def hcheck(status):
        if status != 0:
            msg = _host().gtnh_last_error().decode("utf-8", "replace")
            raise _EXC.get(status, GtnError)(msg)

    def _host_unary(name, *extra):
        def one(g, *args):
            h = C.c_void_p()
            hcheck(getattr(_host(), name)(g._h, *args, C.byref(h)))
            return Graph._from_handle(h.value)
        return one

    def _host_nary(name):
        def one(graphs):
            graphs = list(graphs)
            arr = (C.c_void_p * max(len(graphs), 1))(*[g._h for g in graphs])
            h = C.c_void_p()
            hcheck(getattr(_host(), name)(arr, len(graphs), C.byref(h)))
            return Graph._from_handle(h.value)
        return one

    _clone1 = _host_unary("gtnh_clone")
    _closure1 = _host_unary("gtnh_closure")
    _remove1 = _host_unary("gtnh_remove")
    _concat1 = _host_nary("gtnh_concat")
    _union1 = _host_nary("gtnh_union")

    def clone(g, projection=0):
        """clone(g) (_functions.cpp:78-83); lists map element-wise"""
        if _is_seq(g):
            return [_clone1(x, int(projection)) for x in g]
        return _clone1(g, int(projection))

    def project_input(g):
        return [_clone1(x, 1) for x in g] if _is_seq(g) else _clone1(g, 1)

    def project_output(g):
        return [_clone1(x, 2) for x in g] if _is_seq(g) else _clone1(g, 2)

    def closure(g):
        return [_closure1(x) for x in g] if _is_seq(g) else _closure1(g)

    def _bcast(seq, n):
        seq = list(seq)
        if len(seq) == n:
            return seq
        if len(seq) == 1:
            return seq * n
        raise RuntimeError("parallelMap getIdxOrBroadcast got invalid size or unbroadcastable vector")

    def concat(a, b=None):
        """concat(g1, g2) / concat(graphs1, graphs2) / concat(graphs) / concat(list of lists)
        (_functions.cpp:36-68)"""
        if b is not None:
            if _is_seq(a) or _is_seq(b):
                la = list(a) if _is_seq(a) else [a]
                lb = list(b) if _is_seq(b) else [b]
                n = max(len(la), len(lb))
                return [_concat1([x, y]) for x, y in zip(_bcast(la, n), _bcast(lb, n))]
            return _concat1([a, b])
        if len(a) and _is_seq(a[0]):
            return [_concat1(x) for x in a]
        return _concat1(a)

    def union(graphs):
        """union(graphs) / union(list of lists) (_functions.cpp:221-233)"""
        if len(graphs) and _is_seq(graphs[0]):
            return [_union1(x) for x in graphs]
        return _union1(graphs)

    def remove(g, ilabel=None, olabel=None, label=None, labels=None):
        """remove(g, label=epsilon) / remove(g, ilabel, olabel) / remove(graphs, labels=[epsilon])
        (_functions.cpp:179-203)"""
        if _is_seq(g):
            lab = labels if labels is not None else (ilabel if ilabel is not None else [ns.epsilon])
            lab = list(lab) if _is_seq(lab) else [lab]
            n = max(len(g), len(lab))
            return [_remove1(x, int(l), int(l)) for x, l in zip(_bcast(g, n), _bcast(lab, n))]
        if label is not None:
            ilabel = olabel = label
        if ilabel is None:
            ilabel = ns.epsilon
        if olabel is None:
            olabel = ilabel
        return _remove1(g, int(ilabel), int(olabel))

    def sample(g, max_length=1000):
        h = C.c_void_p()
        hcheck(_host().gtnh_sample(g._h, int(max_length), C.byref(h)))
        return Graph._from_handle(h.value)

    def rand_equivalent(g1, g2, num_samples=1000, tol=1e-4, max_length=1000):
        v = C.c_int()
        hcheck(_host().gtnh_rand_equivalent(g1._h, g2._h, int(num_samples), float(tol), int(max_length), C.byref(v)))
        return bool(v.value)

    def load(file_name):
        h = C.c_void_p()
        hcheck(_host().gtnh_load(str(file_name).encode(), C.byref(h)))
        return Graph._from_handle(h.value)

    def save(file_name, graph):
        hcheck(_host().gtnh_save(str(file_name).encode(), graph._h))

    def loadtxt(file_name):
        h = C.c_void_p()
        hcheck(_host().gtnh_loadtxt(str(file_name).encode(), C.byref(h)))
        return Graph._from_handle(h.value)

    def savetxt(file_name, graph):
        hcheck(_host().gtnh_savetxt(str(file_name).encode(), graph._h))

    def write_dot(g, file_name, isymbols={}, osymbols={}):
        def table(m):
            keys = (C.c_int * max(len(m), 1))(*[int(k) for k in m])
            names = (C.c_char_p * max(len(m), 1))(*[str(v).encode() for v in m.values()])
            return keys, names, len(m)
        ik, inames, ni = table(isymbols)
        ok, onames, no = table(osymbols)
        hcheck(_host().gtnh_write_dot(g._h, str(file_name).encode(), ik, inames, ni, ok, onames, no))

    def draw(graph, file_name, isymbols={}, osymbols={}):
        """bindings/python/gtn/__init__.py:22-26: dot -> picture through graphviz"""
        import os
        import subprocess
        import tempfile
        ext = os.path.splitext(file_name)[1]
        with tempfile.NamedTemporaryFile() as tmpf:
            write_dot(graph, tmpf.name, isymbols, osymbols)
            subprocess.check_call(["dot", "-T" + ext[1:], tmpf.name, "-o", file_name])

    for _n, _f in (("clone", clone), ("project_input", project_input), ("project_output", project_output),
                   ("closure", closure), ("concat", concat), ("union", union), ("remove", remove),
                   ("sample", sample), ("rand_equivalent", rand_equivalent), ("load", load), ("save", save),
                   ("loadtxt", loadtxt), ("savetxt", savetxt), ("write_dot", write_dot), ("draw", draw)):
        setattr(ns, _n, _f)

    # ---------------------------------------------------------------- functions
    def _unary(single, batched):
        def fn(g):
            if _is_seq(g):
                n = len(g)
                out = (C.c_void_p * n)()
                if n:
                    check(batched(_harr(g), n, out))
                return _wrap_many(out, n)
            h = C.c_void_p()
            check(single(g._h, C.byref(h)))
            return Graph._from_handle(h.value)
        return fn

    def _binary(single, batched):
        def fn(a, b):
            if _is_seq(a) or _is_seq(b):
                la = list(a) if _is_seq(a) else [a]
                lb = list(b) if _is_seq(b) else [b]
                n = max(len(la), len(lb))
                out = (C.c_void_p * n)()
                if n:
                    check(batched(_harr(la), len(la), _harr(lb), len(lb), out))
                return _wrap_many(out, n)
            h = C.c_void_p()
            check(single(a._h, b._h, C.byref(h)))
            return Graph._from_handle(h.value)
        return fn

    ns.negate = _unary(lib.gtnx_negate, lib.gtnx_negate_n)
    ns.add = _binary(lib.gtnx_add, lib.gtnx_add_n)
    ns.subtract = _binary(lib.gtnx_subtract, lib.gtnx_subtract_n)
    ns.compose = _binary(lib.gtnx_compose, lib.gtnx_compose_n)
    ns.intersect = _binary(lib.gtnx_intersect, lib.gtnx_intersect_n)
    ns.forward_score = _unary(lib.gtnx_forward_score, lib.gtnx_forward_score_n)
    ns.viterbi_score = _unary(lib.gtnx_viterbi_score, lib.gtnx_viterbi_score_n)
    ns.viterbi_path = _unary(lib.gtnx_viterbi_path, lib.gtnx_viterbi_path_n)

    def backward(g, grad_or_retain=None, retain_graph=False):
        """backward(g, retain_graph=False) / backward(g, grad, retain_graph=False);
        lists run batched (bindings/python/gtn/_autograd.cpp)."""
        grad = None
        if isinstance(grad_or_retain, Graph):
            grad = grad_or_retain
        elif grad_or_retain is not None:
            retain_graph = grad_or_retain
        if _is_seq(g):
            # backward(graphs, retain_graphs=[0]) / backward(graphs, grads, retain_graphs=[0]): parallelMap
            # with size-1 lists broadcast (_autograd.cpp:27-60)
            grads = None
            if _is_seq(grad_or_retain) and grad_or_retain and isinstance(grad_or_retain[0], Graph):
                grads = list(grad_or_retain)
            elif _is_seq(grad_or_retain):
                retain_graph = grad_or_retain
            if grads is not None:
                rl = list(retain_graph) if _is_seq(retain_graph) else [retain_graph]
                n = max(len(g), len(grads), len(rl))
                for x, gr, r in zip(_bcast(g, n), _bcast(grads, n), _bcast(rl, n)):
                    check(lib.gtnx_backward_with_grad(x._h, gr._h, int(bool(r))))
                return
            if _is_seq(retain_graph):
                retain_graph = retain_graph[0] if retain_graph else False
            if len(g):
                check(lib.gtnx_backward_n(_harr(g), len(g), int(bool(retain_graph))))
            return
        if grad is not None:
            check(lib.gtnx_backward_with_grad(g._h, grad._h, int(bool(retain_graph))))
        else:
            check(lib.gtnx_backward(g._h, int(bool(retain_graph))))

    ns.backward = backward

    def scalar_graph(val, calc_grad=True):
        h = C.c_void_p()
        check(lib.gtnx_scalar_graph(float(val), int(bool(calc_grad)), C.byref(h)))
        return Graph._from_handle(h.value)

    def linear_graph(M, N, calc_grad=True):
        h = C.c_void_p()
        check(lib.gtnx_linear_graph(int(M), int(N), int(bool(calc_grad)), C.byref(h)))
        return Graph._from_handle(h.value)

    def linear_graph_n(B, M, N, device_weights, calc_grad=True):
        """B linear graphs with weights copied from one device tensor [B, M, N]"""
        out = (C.c_void_p * B)()
        check(lib.gtnx_linear_graph_n(B, M, N, int(bool(calc_grad)),
                                      _as_dev_ptr(device_weights), out))
        return _wrap_many(out, B)

    ns.scalar_graph = scalar_graph
    ns.linear_graph = linear_graph
    ns.linear_graph_n = linear_graph_n

    def equal(a, b):
        v = C.c_int()
        check(lib.gtnx_equal(a._h, b._h, C.byref(v)))
        return bool(v.value)

    def isomorphic(a, b):
        v = C.c_int()
        check(lib.gtnx_isomorphic(a._h, b._h, C.byref(v)))
        return bool(v.value)

    ns.equal = equal
    ns.isomorphic = isomorphic

    def items(graphs):
        """item() of many scalar graphs with one device->host copy"""
        n = len(graphs)
        out = np.empty(n, dtype=np.float32)
        if n:
            check(lib.gtnx_items_n(_harr(graphs), n, out.ctypes.data))
        return out

    def items_to_device(graphs, device_out):
        check(lib.gtnx_items_device_n(_harr(graphs), len(graphs), _as_dev_ptr(device_out)))

    def grads_to_device(graphs, device_out, offsets):
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        check(lib.gtnx_grads_device_n(_harr(graphs), len(graphs), _as_dev_ptr(device_out),
                                      off.ctypes.data))

    ns.items = items
    ns.items_to_device = items_to_device
    ns.grads_to_device = grads_to_device

    # ---------------------------------------------------------------- compiled LM graphs (gtnx_lm_graph_*)
    class _LmGraphInfo(C.Structure):
        _fields_ = [("num_states", C.c_int64), ("num_arcs", C.c_int64), ("start_state", C.c_int32),
                    ("longest_epsilon_chain", C.c_int32)]

    class LmGraph:
        """A language model held as a Graph, compiled for `Batch.ctc_beam_decode(lm=...)` and
        `Batch.asg_beam_decode(lm=...)` (gtnx_lm_graph_create; DESIGN sections 30 and 31): a deterministic acceptor
        with back-off (failure) arcs -- an n-gram model in ARPA form, or a lexicon or grammar acceptor that forbids
        label sequences.  A SNAPSHOT of the graph's input labels and weights at this moment: later changes of `graph`
        are not seen, and there is no autograd.  Output labels and accept flags are ignored (an n-gram acceptor accepts
        everywhere; end-of-sentence handling is out of scope).  The arcs need not be sorted.  Compiling and `walk` are
        host work and need no GPU; the first decode uploads the compiled form.
        ValueError, nothing is repaired: no start node or several, two arcs with one input label out of a node, several
        epsilon arcs out of a node, an epsilon chain that is cyclic or longer than 8 arcs, a label below -1, more than
        2^24 nodes."""

        __slots__ = ("_h", "__weakref__")

        def __init__(self, graph):
            self._h = None
            h = C.c_void_p()
            check(lib.gtnx_lm_graph_create(graph._h, C.byref(h)))
            self._h = h.value

        def destroy(self):
            """let go of the compiled form now; a decode with this object is refused from here on"""
            h, self._h = self._h, None
            if h:
                check(lib.gtnx_lm_graph_destroy(h))

        def __del__(self):
            h = getattr(self, "_h", None)
            if h:
                try:
                    lib.gtnx_lm_graph_destroy(h)
                except Exception:
                    pass
                self._h = None

        def walk(self, state, label):
            """(weight, next_state) of `label` from `state`, failure-arc semantics: the arc labelled `label` if the
            state has one, else its epsilon arc and the same question at its destination; the weight is the float32
            sum of the walked weights in walk order.  A forbidden label gives (-inf, -1)."""
            w, nx = C.c_float(), C.c_int()
            check(lib.gtnx_lm_graph_walk(self._h, int(state), int(label), C.byref(w), C.byref(nx)))
            return w.value, nx.value

        def info(self):
            """dict: num_states, num_arcs (epsilon arcs included), start_state, longest_epsilon_chain"""
            i = _LmGraphInfo()
            check(lib.gtnx_lm_graph_info(self._h, C.byref(i)))
            return {k: int(getattr(i, k)) for k, _ in _LmGraphInfo._fields_}

    ns.LmGraph = LmGraph

    # ---------------------------------------------------------------- batch records (gtnx_batch_*)
    class Batch:
        """B graphs held as one record: what the list forms of the functions return when
        nobody looks at the elements (one object and one tape node per call).  `b[i]` is
        element i as an ordinary Graph.  The module-level functions (intersect, forward_score,
        subtract, backward, ...) accept Batch arguments."""

        __slots__ = ("_h", "_keep", "__weakref__")  # (_keep: a caller's tensor the record borrows, subtract_into)

        def __init__(self, graphs=None):
            self._h = None
            if graphs is not None:
                graphs = list(graphs)
                h = C.c_void_p()
                check(lib.gtnx_batch_from_graphs(_harr(graphs), len(graphs), C.byref(h)))
                self._h = h.value

        @classmethod
        def _from_handle(cls, h):
            b = cls.__new__(cls)
            b._h = h
            return b

        @classmethod
        def ctc_targets(cls, targets, blank=0, calc_grad=True):
            """CTC target acceptors (benchmarks/ctc.cpp:40-58) of label sequences, built on the device"""
            lens = np.asarray([len(t) for t in targets], dtype=np.int32)
            flat = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int32).reshape(-1) for t in targets])
                                        if len(targets) else np.zeros(0, np.int32), dtype=np.int32)
            h = C.c_void_p()
            check(lib.gtnx_batch_ctc_targets(flat.ctypes.data, lens.ctypes.data, len(lens), int(blank),
                                             int(bool(calc_grad)), C.byref(h)))
            return cls._from_handle(h.value)

        @classmethod
        def asg_force_align(cls, targets, transitions, n_labels):
            """compose(forceAlign(target), transitions) of examples/asg.cpp:50-68 for every label sequence, built on
            the device; `transitions`: a Graph in the arc layout of examples/asg.cpp:36-47 over n_labels labels"""
            lens = np.asarray([len(t) for t in targets], dtype=np.int32)
            flat = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int32).reshape(-1) for t in targets])
                                        if len(targets) else np.zeros(0, np.int32), dtype=np.int32)
            h = C.c_void_p()
            check(lib.gtnx_batch_asg_force_align(flat.ctypes.data, lens.ctypes.data, len(lens), transitions._h,
                                                 int(n_labels), C.byref(h)))
            return cls._from_handle(h.value)

        @classmethod
        def linear(cls, B, M, N, device_weights, calc_grad=True, borrow=False, rows=None):
            """B linear graphs over one device tensor [B, M, N]; borrow: read in place; rows: per-element row counts
            of a padded tensor (1 .. M) -- element b is linear_graph(rows[b], N) over the first rows[b] rows of its
            slab, and its gradient keeps the [M, N] layout with zeros in the pad rows"""
            h = C.c_void_p()
            if rows is not None:
                r = np.ascontiguousarray([int(v) for v in rows], dtype=np.int32)
                if r.shape != (int(B),):
                    raise ValueError(f"Batch.linear: {r.size} row counts for a batch of {int(B)}")
                check(lib.gtnx_batch_linear_rows(int(B), int(M), int(N), r.ctypes.data, int(bool(calc_grad)),
                                                 _as_dev_ptr(device_weights), int(bool(borrow)), C.byref(h)))
                return cls._from_handle(h.value)
            check(lib.gtnx_batch_linear(int(B), int(M), int(N), int(bool(calc_grad)), _as_dev_ptr(device_weights),
                                        int(bool(borrow)), C.byref(h)))
            return cls._from_handle(h.value)

        def __del__(self):
            h, self._h = getattr(self, "_h", None), None
            if h:
                try:
                    lib.gtnx_batch_destroy(h)
                except Exception:
                    pass

        def __len__(self):
            v = C.c_int()
            check(lib.gtnx_batch_size(self._h, C.byref(v)))
            return v.value

        def __getitem__(self, i):
            h = C.c_void_p()
            check(lib.gtnx_batch_get(self._h, int(i), C.byref(h)))
            return Graph._from_handle(h.value)

        def items(self):
            out = np.empty(len(self), dtype=np.float32)
            if len(out):
                check(lib.gtnx_batch_items(self._h, out.ctypes.data))
            return out

        def items_to_device(self, device_out):
            check(lib.gtnx_batch_items_device(self._h, _as_dev_ptr(device_out)))

        def bind_grads(self, device_out, offsets):
            off = np.ascontiguousarray(offsets, dtype=np.int64)
            check(lib.gtnx_batch_grads_bind_device(self._h, _as_dev_ptr(device_out), off.ctypes.data))

        def grads_to_device(self, device_out, offsets):
            off = np.ascontiguousarray(offsets, dtype=np.int64)
            check(lib.gtnx_batch_grads_device(self._h, _as_dev_ptr(device_out), off.ctypes.data))

        def viterbi_align(self, labels_out, tokens_out=None, scores_out=None, frames=None, row_stride=None):
            """forced alignment with the results left on the device (gtnx_batch_viterbi_align): row b of `labels_out`
            (int32 CUDA tensor [B, >= T], or a device address with `row_stride` entries between rows) gets the label of every frame of
            element b's best path, -1 past the path and everywhere when no path exists; `tokens_out` the index into
            the label sequence (-1 on blank frames), `scores_out` (float32 [B]) the path scores; `frames`: per-element
            frame counts.  A composition of Batch.ctc_targets with Batch.linear is one launch with no copy back and no
            wait, and so is a composition of Batch.asg_force_align with Batch.linear over the same alphabet, in either
            argument order (there `tokens_out` = index into the label sequence, never -1 inside a path: ASG has no
            blanks); other batches go through viterbi_path (tokens_out and frames are errors there)."""
            n = len(self)
            stride = _row_tensors("viterbi_align", "labels_out and tokens_out", (labels_out, tokens_out), n, row_stride,
                                  "T")
            fr, fr_ptr = _frames_arg("viterbi_align", frames, n)
            check(lib.gtnx_batch_viterbi_align(self._h, fr_ptr, _as_dev_ptr(labels_out), stride, _opt_ptr(tokens_out),
                                               _opt_ptr(scores_out)))

        def viterbi_decode(self, transitions, labels_out, scores_out=None, frames=None, collapsed_out=None,
                           lengths_out=None, row_stride=None):
            """viterbi_path(compose(element b, transitions)) of the whole batch against ONE shared graph, results left
            on the device (gtnx_batch_viterbi_decode): row b of `labels_out` (int32 CUDA tensor [B, >= M], or a device
            address with `row_stride` entries between rows) gets the label of every frame t < T_b and -1 from T_b to
            the row's width M; `scores_out` (float32 [B]) the path scores; `collapsed_out` (int32, rows like
            labels_out) the labels with runs of equal consecutive frames merged, then -1; `lengths_out` (int32 [B],
            needs collapsed_out) how many; `frames`: T_b per element (0 .. M, at most the rows the batch carries;
            None: those rows).  Without an accepting path (T_b = 0 included): entries -1, score -inf, length 0.
            A Batch.linear against an asg-transitions-shaped graph of 8 .. 1024 nodes (7 .. 1023 labels) is ONE sweep
            of the padded batch and one launch, with no copy back and no wait; the pad rows never change a bit of any
            output; exact ties: first accept node, then the smallest source node.  Other graphs / batches go through
            viterbi_path and one upload (`frames` is an error there)."""
            n = len(self)
            stride = _row_tensors("viterbi_decode", "labels_out and collapsed_out", (labels_out, collapsed_out), n,
                                  row_stride, "M")
            if lengths_out is not None and collapsed_out is None:
                raise ValueError("viterbi_decode: lengths_out needs collapsed_out")
            fr, fr_ptr = _frames_arg("viterbi_decode", frames, n)
            check(lib.gtnx_batch_viterbi_decode(self._h, transitions._h, fr_ptr, _as_dev_ptr(labels_out), stride,
                                                _opt_ptr(scores_out), _opt_ptr(collapsed_out), _opt_ptr(lengths_out)))

        def linear_decode(self, labels_out, scores_out=None, frames=None, blank=-1, collapsed_out=None,
                          starts_out=None, lengths_out=None, row_stride=None):
            """viterbi_path(element b) of a batch of chains plus the CTC collapse, results left on the device
            (gtnx_batch_linear_decode): row b of `labels_out` (int32 CUDA tensor [B, >= M], or a device address with
            `row_stride` entries between rows) gets the first label holding the maximum of every frame t < T_b (the
            smallest label among equal maxima; NaN and -inf are never taken) and -1 from T_b to the row's width M;
            `scores_out` (float32 [B]) the path scores, the float32 sum of the maxima in frame order; `collapsed_out`
            (int32, rows like labels_out) the labels with repeats merged and `blank` dropped (blank < 0: nothing is
            dropped), then -1; `starts_out` (rows alike, needs collapsed_out) the first frame of each; `lengths_out`
            (int32 [B], needs collapsed_out) how many; `frames`: T_b per element (0 .. M, at most the rows the batch
            carries; None: those rows).  A frame with nothing above -inf leaves no path: entries -1, score -inf,
            length 0; T_b = 0 likewise (a chain without frames has no accepting node).
            A Batch.linear is two launches with no copy back and no wait; rows from T_b on are never read.  Other
            batches go through viterbi_path and one upload (`frames` is an error there)."""
            n = len(self)
            stride = _row_tensors("linear_decode", "labels_out, collapsed_out and starts_out",
                                  (labels_out, collapsed_out, starts_out), n, row_stride, "M")
            if (lengths_out is not None or starts_out is not None) and collapsed_out is None:
                raise ValueError("linear_decode: lengths_out and starts_out need collapsed_out")
            fr, fr_ptr = _frames_arg("linear_decode", frames, n)
            check(lib.gtnx_batch_linear_decode(self._h, fr_ptr, int(blank), _as_dev_ptr(labels_out), stride,
                                               _opt_ptr(scores_out), _opt_ptr(collapsed_out), _opt_ptr(starts_out),
                                               _opt_ptr(lengths_out)))

        def _nbest_outputs(self, who, tokens_out, nbest, row_stride, flat):
            """the row stride of the [B, nbest, >= M] token rows of a beam search, with the outputs checked where they are
            tensors; `flat`: (tensor, dtype, text) of its [B, nbest] outputs"""
            n = len(self)
            stride = row_stride
            t = tokens_out
            if t is not None and hasattr(t, "data_ptr"):
                if (str(t.dtype) != "torch.int32" or t.dim() != 3 or t.shape[0] < n or t.shape[1] != int(nbest)
                        or (t.shape[2] > 1 and t.stride(2) != 1) or (n > 1 and t.stride(0) != t.shape[1] * t.stride(1))):
                    raise ValueError(f"{who}: tokens_out must be an int32 tensor [B, nbest, M] with contiguous "
                                     "rows, equally spaced")
                if stride is not None and t.stride(1) != stride:
                    raise ValueError(f"{who}: row_stride is not the row stride of tokens_out")
                stride = t.stride(1)
                m, c = C.c_int(-1), C.c_int(-1)
                check(lib.gtnx_batch_linear_shape(self._h, C.byref(m), C.byref(c)))
                if t.shape[2] < m.value:  # (the kernel writes M entries of every row, whatever lies behind a view)
                    raise ValueError(f"{who}: tokens_out has rows of {t.shape[2]} entries, the batch has "
                                     f"{m.value} rows")
            if stride is None:
                raise ValueError(f"{who}: a device address needs row_stride")
            for o, dt, what in flat:
                if o is not None and hasattr(o, "data_ptr") and (str(o.dtype) != dt or not o.is_contiguous()
                                                                 or o.numel() < n * int(nbest)):
                    raise ValueError(f"{who}: {what} contiguous tensor [B, nbest]")
            return stride

        def ctc_sample(self, tokens_out, lengths_out, logq_out=None, labels_out=None, frames=None, blank=0,
                       num_samples=4, seed=0, temperature=1.0, row_stride=None):
            """`num_samples` label sequences per utterance drawn from the CTC posterior of a Batch.linear, results left on
            the device (gtnx_batch_ctc_sample; DESIGN section 32 holds the contract).  Frame t < T_b of sample k takes
            label c with probability exp(x[b, t, c] / temperature) / Z[b, t], independently -- only finite entries carry
            mass -- by inverse CDF in label order against a Philox4x32-10 uniform keyed by `seed` and counted by
            (t, b, k): the same seed gives the same bytes whatever the strides, the other utterances' frame counts or
            the pad rows hold, and the first N samples of a larger call are those of a call with N.
            `tokens_out` (int32 CUDA tensor [B, num_samples, >= M] with contiguous rows, or a device address of
            [B][num_samples][row_stride]) gets every alignment with repeats merged and `blank` dropped (blank = -1:
            repeats merged only), -1 from its length to the row's width M -- the layout `ctc_beam_decode` writes, so
            `ctc_score`, `edit_distance` and `ctc_token_align` take it as it is; `lengths_out` (int32
            [B, num_samples]) the lengths; `logq_out` (float32 [B, num_samples], optional) the log-probability of each
            drawn alignment, sum_t (x / temperature - log Z), float32 in frame order; `labels_out` (rows like
            tokens_out, optional) the frame labels, -1 from T_b on.  A frame without a finite entry, or T_b = 0: -1
            rows, length 0, logq -inf for every sample of that utterance.  `num_samples` 1 .. 1024, `temperature`
            finite and > 0, `seed` 0 .. 2^64 - 1; `frames`: T_b per element (0 .. M, at most the rows the batch
            carries; None: those rows).  Two launches with no copy back and no wait; rows from T_b on are never read.
            Any batch but a Batch.linear is an error: there is no other route."""
            n = len(self)
            seed = int(seed)
            if not 0 <= seed < (1 << 64):
                raise ValueError("ctc_sample: seed must be in 0 .. 2^64 - 1")
            stride = self._nbest_outputs("ctc_sample", tokens_out, num_samples, row_stride,
                                         ((lengths_out, "torch.int32", "lengths_out must be an int32"),
                                          (logq_out, "torch.float32", "logq_out must be a float32")))
            if labels_out is not None and hasattr(labels_out, "data_ptr"):
                if self._nbest_outputs("ctc_sample", labels_out, num_samples, None, ()) != stride:
                    raise ValueError("ctc_sample: labels_out must have the row stride of tokens_out")
            fr, fr_ptr = _frames_arg("ctc_sample", frames, n)
            check(lib.gtnx_batch_ctc_sample(self._h, fr_ptr, int(blank), int(num_samples), seed, float(temperature),
                                            _opt_ptr(tokens_out), int(stride), _opt_ptr(lengths_out),
                                            _opt_ptr(logq_out), _opt_ptr(labels_out)))

        def asg_beam_decode(self, tokens_out, lengths_out, scores_out, frames, table, beam_size=16, cutoff_top_n=16,
                            nbest=1, row_stride=None, lm=None, lm_weight=1.0, insertion_bonus=0.0, am_scores_out=None):
            """ASG prefix beam search with N-best output over a Batch.linear, results left on the device
            (gtnx_batch_asg_beam_decode; DESIGN section 27 holds the contract).  The hypotheses are the label sequences
            without equal neighbours -- what `viterbi_decode`'s collapsed rows can hold -- each summed over all of its
            alignments under emissions o transitions: unpruned, a hypothesis's score is `asg_score` of its tokens.
            `tokens_out` (int32 CUDA tensor [B, nbest, >= M] with contiguous rows, or a device address of
            [B][nbest][row_stride]) gets the labels of the `nbest` best of every utterance, best first, -1 from each
            one's length to the row's width M; `lengths_out` (int32 [B, nbest]) their lengths; `scores_out` (float32
            [B, nbest]) their log scores.  Slots without a hypothesis (fewer than nbest prefixes, a frame with nothing
            above -inf, T_b = 0): -1, 0, -inf.  `table`: float32 CUDA tensor [C + C * C] or a device address -- entry c
            is start[c], entry C + i * C + j is transitions[i, j], label j followed by label i
            (`torch_loss._asg_weights(start, transitions)`, the table `asg_score` takes); an entry that is not finite
            forbids its bigram or first label.  `beam_size` 1 .. 64 prefixes are kept, a frame offers its `cutoff_top_n`
            (1 .. 32) best labels, for stays as well as extensions; `frames`: T_b per element (0 .. M, at most the rows
            the batch carries; None: those rows).  Two launches with no copy back and no wait; rows from T_b on are never
            read.  Any batch but a Batch.linear is an error: there is no other route.
            `lm` (an `LmGraph`; None: no language model, the call above) fuses a language model held as a graph -- a
            lexicon, a grammar, an n-gram model -- into the ranking (gtnx_batch_asg_beam_decode_graph; DESIGN section
            31); `table` stays the criterion's own.  A prefix then also carries L and its state in the graph: an
            extension walks (state, label) -- failure-arc semantics, see `LmGraph.walk` -- and adds lm_weight * (the
            walk's weight) + insertion_bonus to L; a label the walk forbids, or whose term is not finite, is dropped.
            Candidates rank by acoustic score + L; stays, merging and the token sets stay acoustic.  `scores_out` then
            gets acoustic + L and `am_scores_out` (float32 [B, nbest], optional) the acoustic score alone -- unpruned,
            `asg_score` of those tokens; slots without a hypothesis hold -inf in both.  ValueError: an `lm` that is no
            `LmGraph`; `lm_weight`, `insertion_bonus` or `am_scores_out` given without `lm`; a weight or bonus that
            is not finite; a destroyed `LmGraph`."""
            n = len(self)
            if lm is None:
                if lm_weight != 1.0 or insertion_bonus != 0.0 or am_scores_out is not None:
                    raise ValueError("asg_beam_decode: lm_weight, insertion_bonus and am_scores_out need lm")
            else:
                if not isinstance(lm, LmGraph):
                    raise ValueError("asg_beam_decode: lm must be an LmGraph")
                lm_weight, insertion_bonus = float(lm_weight), float(insertion_bonus)
                if not (math.isfinite(lm_weight) and math.isfinite(insertion_bonus)):
                    raise ValueError("asg_beam_decode: lm_weight and insertion_bonus must be finite")
            table = self._asg_score_table("asg_beam_decode", table)
            stride = self._nbest_outputs("asg_beam_decode", tokens_out, nbest, row_stride,
                                         ((lengths_out, "torch.int32", "lengths_out must be an int32"),
                                          (scores_out, "torch.float32", "scores_out must be a float32"),
                                          (am_scores_out, "torch.float32", "am_scores_out must be a float32")))
            fr, fr_ptr = _frames_arg("asg_beam_decode", frames, n)
            if lm is not None:
                # (a destroyed object has no handle: the engine refuses the null one)
                check(lib.gtnx_batch_asg_beam_decode_graph(self._h, fr_ptr, _opt_ptr(table), int(beam_size),
                                                           int(cutoff_top_n), int(nbest), lm._h, lm_weight,
                                                           insertion_bonus, _opt_ptr(tokens_out), int(stride),
                                                           _opt_ptr(lengths_out), _opt_ptr(scores_out),
                                                           _opt_ptr(am_scores_out)))
                return
            check(lib.gtnx_batch_asg_beam_decode(self._h, fr_ptr, _opt_ptr(table), int(beam_size), int(cutoff_top_n),
                                                 int(nbest), _opt_ptr(tokens_out), int(stride), _opt_ptr(lengths_out),
                                                 _opt_ptr(scores_out)))

        def asg_sample(self, tokens_out, lengths_out, table, logq_out=None, labels_out=None, logz_out=None, frames=None,
                       num_samples=4, seed=0, temperature=1.0, row_stride=None):
            """`num_samples` alignments per utterance drawn from the posterior of the ASG model emissions o transitions
            over a Batch.linear, equal neighbours merged, results left on the device (gtnx_batch_asg_sample; DESIGN
            section 34 holds the contract).  ASG frames are not independent, so the call filters forward -- alpha planes
            in a per-frame rescaled form -- and samples backward: frame T_b - 1 from exp(alpha), frame t below it from
            exp(alpha_t[j] + transitions[y_{t+1}, j] / temperature), by inverse CDF in label order against a
            Philox4x32-10 uniform keyed by `seed` and counted by (t, b, k): alignment y comes with probability
            exp(s(y) / temperature - logZ_b).  The same seed gives the same bytes whatever the strides, the other
            utterances' frame counts or the pad rows hold, and the first N samples of a larger call are those of a call
            with N.  `table`: float32 CUDA tensor [C + C * C] or a device address, the table `asg_score` and
            `asg_beam_decode` take (`torch_loss._asg_weights(start, transitions)`); only finite entries, of it and of
            the emissions, carry mass.
            `tokens_out` (int32 CUDA tensor [B, num_samples, >= M] with contiguous rows, or a device address of
            [B][num_samples][row_stride]) gets every alignment with equal neighbours merged, -1 from its length to the
            row's width M -- the layout `asg_beam_decode` writes, so `asg_score`, `edit_distance` and `asg_token_align`
            take it as it is; `lengths_out` (int32 [B, num_samples]) the lengths; `logq_out` (float32 [B, num_samples],
            optional) the log-probability of each drawn alignment, the drawn conditionals' logs added in draw order in
            float32; `labels_out` (rows like tokens_out, optional) the frame labels, -1 from T_b on; `logz_out` (float32
            [B], optional) logZ_b, at temperature 1 the full-connect score of the utterance.  No alignment of finite
            score, or T_b = 0: -1 rows, length 0, logq -inf for every sample of that utterance, logz -inf.
            `num_samples` 1 .. 1024, `temperature` finite and > 0, `seed` 0 .. 2^64 - 1, 1 .. 1024 labels; `frames`:
            T_b per element (0 .. M, at most the rows the batch carries; None: those rows).  No copy back and no wait;
            rows from T_b on are never read.  Any batch but a Batch.linear is an error: there is no other route."""
            n = len(self)
            seed = int(seed)
            if not 0 <= seed < (1 << 64):
                raise ValueError("asg_sample: seed must be in 0 .. 2^64 - 1")
            table = self._asg_score_table("asg_sample", table)
            stride = self._nbest_outputs("asg_sample", tokens_out, num_samples, row_stride,
                                         ((lengths_out, "torch.int32", "lengths_out must be an int32"),
                                          (logq_out, "torch.float32", "logq_out must be a float32")))
            if labels_out is not None and hasattr(labels_out, "data_ptr"):
                if self._nbest_outputs("asg_sample", labels_out, num_samples, None, ()) != stride:
                    raise ValueError("asg_sample: labels_out must have the row stride of tokens_out")
            if logz_out is not None and hasattr(logz_out, "data_ptr"):
                if str(logz_out.dtype) != "torch.float32" or tuple(logz_out.shape) != (n,) or not logz_out.is_contiguous():
                    raise ValueError("asg_sample: logz_out must be a float32 contiguous tensor [B]")
            fr, fr_ptr = _frames_arg("asg_sample", frames, n)
            check(lib.gtnx_batch_asg_sample(self._h, fr_ptr, _opt_ptr(table), int(num_samples), seed,
                                            float(temperature), _opt_ptr(tokens_out), int(stride),
                                            _opt_ptr(lengths_out), _opt_ptr(logq_out), _opt_ptr(labels_out),
                                            _opt_ptr(logz_out)))

        def ctc_beam_decode(self, tokens_out, lengths_out, scores_out, frames=None, blank=0, beam_size=16,
                            cutoff_top_n=16, nbest=1, row_stride=None, lm=None, lm_weight=1.0, insertion_bonus=0.0,
                            am_scores_out=None):
            """CTC prefix beam search with N-best output over a Batch.linear, results left on the device
            (gtnx_batch_ctc_beam_decode; DESIGN section 20 holds the contract): `tokens_out` (int32 CUDA tensor
            [B, nbest, >= M] with contiguous rows, or a device address of [B][nbest][row_stride]) gets the labels of
            the `nbest` best label sequences of every utterance, best first, -1 from each one's length to the row's
            width M; `lengths_out` (int32 [B, nbest]) their lengths; `scores_out` (float32 [B, nbest]) their log
            scores, summed over the alignments the beam kept.  Slots without a hypothesis (fewer than nbest prefixes, a
            frame with nothing above -inf, T_b = 0): -1, 0, -inf.  `beam_size` 1 .. 64 prefixes are kept, a frame
            offers its `cutoff_top_n` (1 .. 32) best labels plus `blank`; `frames`: T_b per element (0 .. M, at most
            the rows the batch carries; None: those rows).  Two launches with no copy back and no wait; rows from T_b
            on are never read.  Any batch but a Batch.linear is an error: there is no other route.
            `lm` (float32 CUDA tensor [C + C * C] or a device address; None: no language model, the call above) fuses
            a bigram over the labels into the ranking (gtnx_batch_ctc_beam_decode_lm): lm[c] scores
            c as first label, lm[C + i * C + j] label j followed by label i -- `torch_loss._asg_weights(start,
            transitions)`.  A prefix carries L = the sum over its labels of lm_weight * lm(...) + insertion_bonus;
            candidates rank by acoustic total + L, a -inf entry forbids its bigram or first label, row pruning stays
            acoustic.  `scores_out` then gets acoustic + L and `am_scores_out` (float32 [B, nbest], optional) the
            acoustic total alone; slots without a hypothesis hold -inf in both.
            `lm` may also be an `LmGraph` (gtnx_batch_ctc_beam_decode_graph): a prefix then carries
            its LM state too, and the table entry of an extension is the weight of the walk of (state, label) through
            the graph -- failure-arc semantics, see `LmGraph.walk`; a label the walk forbids, or whose weight is not
            finite, is dropped.  `blank` is never walked.  Everything else is as with the table."""
            n = len(self)
            if lm is None and am_scores_out is not None:
                raise ValueError("ctc_beam_decode: am_scores_out needs lm")
            if lm is not None and hasattr(lm, "data_ptr"):
                if str(lm.dtype) != "torch.float32" or lm.dim() != 1 or not lm.is_contiguous() or not lm.is_cuda:
                    raise ValueError("ctc_beam_decode: lm must be a float32 contiguous CUDA tensor [C + C * C]")
                m, c = C.c_int(-1), C.c_int(-1)
                check(lib.gtnx_batch_linear_shape(self._h, C.byref(m), C.byref(c)))
                if c.value >= 0 and lm.numel() != c.value + c.value * c.value:
                    raise ValueError(f"ctc_beam_decode: lm has {lm.numel()} entries, {c.value} labels need "
                                     f"{c.value + c.value * c.value}")
            stride = self._nbest_outputs("ctc_beam_decode", tokens_out, nbest, row_stride,
                                         ((lengths_out, "torch.int32", "lengths_out must be an int32"),
                                          (scores_out, "torch.float32", "scores_out must be a float32"),
                                          (am_scores_out, "torch.float32", "am_scores_out must be a float32")))
            fr, fr_ptr = _frames_arg("ctc_beam_decode", frames, n)
            if isinstance(lm, LmGraph):
                # (a destroyed object has no handle: the engine refuses the null one)
                check(lib.gtnx_batch_ctc_beam_decode_graph(self._h, fr_ptr, int(blank), int(beam_size), int(cutoff_top_n),
                                                           int(nbest), lm._h, float(lm_weight), float(insertion_bonus),
                                                           _opt_ptr(tokens_out), int(stride), _opt_ptr(lengths_out),
                                                           _opt_ptr(scores_out), _opt_ptr(am_scores_out)))
                return
            if lm is not None:
                check(lib.gtnx_batch_ctc_beam_decode_lm(self._h, fr_ptr, int(blank), int(beam_size), int(cutoff_top_n),
                                                        int(nbest), _opt_ptr(lm), float(lm_weight),
                                                        float(insertion_bonus), _opt_ptr(tokens_out), int(stride),
                                                        _opt_ptr(lengths_out), _opt_ptr(scores_out),
                                                        _opt_ptr(am_scores_out)))
                return
            check(lib.gtnx_batch_ctc_beam_decode(self._h, fr_ptr, int(blank), int(beam_size), int(cutoff_top_n),
                                                 int(nbest), _opt_ptr(tokens_out), int(stride), _opt_ptr(lengths_out),
                                                 _opt_ptr(scores_out)))

        def _ctc_score_args(self, who, tokens, lengths, frames, N, L, row_stride, max_length):
            """(frames array or None, tokens address, row stride, lengths address, N, L, max_length) of a ctc_score call"""
            n = len(self)
            if tokens is not None and hasattr(tokens, "data_ptr"):
                t = tokens
                if str(t.dtype) != "torch.int32" or t.dim() != 3 or t.shape[0] != n:
                    raise ValueError(f"{who}: tokens must be an int32 tensor [B, N, L]")
                if ((t.shape[2] > 1 and t.stride(2) != 1)
                        or (t.shape[0] > 1 and t.shape[1] > 1 and t.stride(0) != t.shape[1] * t.stride(1))):
                    raise ValueError(f"{who}: tokens must have contiguous rows, equally spaced")
                rows = t.stride(1) if t.shape[1] > 1 else (t.stride(0) if t.shape[0] > 1 else max(t.shape[2], 1))
                for name, given, have in (("N", N, t.shape[1]), ("L", L, t.shape[2]), ("row_stride", row_stride, rows)):
                    if given is not None and int(given) != int(have):
                        raise ValueError(f"{who}: {name} = {given} is not what tokens says ({have})")
                N, L, row_stride = t.shape[1], t.shape[2], rows
                if hasattr(t, "is_cuda") and not t.is_cuda:
                    raise ValueError(f"{who}: tokens must be a CUDA tensor")
            if N is None or L is None or row_stride is None:
                raise ValueError(f"{who}: a device address needs N, L and row_stride")
            N, L = int(N), int(L)
            if lengths is not None and hasattr(lengths, "data_ptr"):
                if str(lengths.dtype) != "torch.int32" or not lengths.is_contiguous() or lengths.numel() != n * N:
                    raise ValueError(f"{who}: lengths must be an int32 contiguous tensor [B, N]")
                if hasattr(lengths, "is_cuda") and not lengths.is_cuda:
                    raise ValueError(f"{who}: lengths must be a CUDA tensor")
            fr, _ = _frames_arg(who, frames, n)
            if max_length is None:
                m, c = C.c_int(-1), C.c_int(-1)
                check(lib.gtnx_batch_linear_shape(self._h, C.byref(m), C.byref(c)))
                max_length = max(1, min(L, m.value if m.value >= 0 else L, 4096))
            return fr, tokens, int(row_stride), lengths, N, L, int(max_length)

        def ctc_score(self, tokens, lengths, scores_out, frames=None, blank=0, max_length=None, N=None, L=None,
                      row_stride=None):
            """The exact log score of all B * N device-resident hypotheses under the slabs of a Batch.linear, results
            left on the device (gtnx_batch_ctc_score; DESIGN section 22 holds the contract): scores_out[b, k] =
            forwardScore(ctcGraph(tokens[b, k, :len], blank) o emissions_b[:T_b]) with len = clamp(lengths[b, k], 0, L),
            nothing subtracted.  `tokens`: int32 CUDA tensor [B, N, L] with contiguous, equally spaced rows, or a device
            address with N, L and row_stride (elements between rows, >= L); `lengths`: int32 [B, N], contiguous -- they
            stay on the device; `scores_out`: float32 [B, N]; `frames`: T_b per element (0 .. M) or None; `max_length`
            (1 .. 4096, default min(L, M, 4096)): the bound on len that sizes LDS -- longer hypotheses score -inf, as do
            ones that do not fit, tokens outside 0 .. C - 1 inside a length, and T_b == 0.  A slot without a hypothesis
            (length 0, tokens -1) scores as the empty sequence.  One launch, no copy back and no wait."""
            fr, tok, stride, ln, N, L, U = self._ctc_score_args("ctc_score", tokens, lengths, frames, N, L, row_stride,
                                                                max_length)
            if scores_out is not None and hasattr(scores_out, "data_ptr"):
                if (str(scores_out.dtype) != "torch.float32" or not scores_out.is_contiguous()
                        or scores_out.numel() != len(self) * N):
                    raise ValueError("ctc_score: scores_out must be a float32 contiguous tensor [B, N]")
                if len(self) * N == 0:
                    return
            check(lib.gtnx_batch_ctc_score(self._h, fr.ctypes.data if fr is not None else None, int(blank), _opt_ptr(tok),
                                           stride, _opt_ptr(ln), N, L, U, _opt_ptr(scores_out)))

        def ctc_score_grad(self, tokens, lengths, weights, grad_out, frames=None, blank=0, max_length=None, N=None,
                           L=None, row_stride=None):
            """grad_out[b, t, c] = sum over k of weights[b, k] * d score[b, k] / d emissions[b, t, c] for the scores of
            `ctc_score` (gtnx_batch_ctc_score_grad): `weights` float32 [B, N] on the device, `grad_out` float32
            [B, M, C], every element written (zeros where nothing lands, rows from T_b on included) -- except that a call
            without pairs (B * N == 0) writes nothing.  Pairs with a -inf score or a weight of exactly 0 add nothing.
            Stateless: the alpha rows are recomputed into pooled scratch (sliced beyond 256 MiB, same bits); the sums are
            taken in a fixed order without atomics, so the result has the same bits run to run."""
            fr, tok, stride, ln, N, L, U = self._ctc_score_args("ctc_score_grad", tokens, lengths, frames, N, L,
                                                                row_stride, max_length)
            for o, what in ((weights, "weights must be a float32 contiguous tensor [B, N]"),
                            (grad_out, "grad_out must be a float32 contiguous tensor [B, M, C]")):
                if o is not None and hasattr(o, "data_ptr"):
                    if str(o.dtype) != "torch.float32" or not o.is_contiguous():
                        raise ValueError(f"ctc_score_grad: {what}")
            if weights is not None and hasattr(weights, "data_ptr") and weights.numel() != len(self) * N:
                raise ValueError("ctc_score_grad: weights must be a float32 contiguous tensor [B, N]")
            if grad_out is not None and hasattr(grad_out, "data_ptr"):
                m, c = C.c_int(-1), C.c_int(-1)
                check(lib.gtnx_batch_linear_shape(self._h, C.byref(m), C.byref(c)))
                if m.value >= 0 and grad_out.numel() != len(self) * m.value * c.value:
                    raise ValueError("ctc_score_grad: grad_out must be a float32 contiguous tensor [B, M, C]")
                if len(self) * N == 0:
                    return
            check(lib.gtnx_batch_ctc_score_grad(self._h, fr.ctypes.data if fr is not None else None, int(blank),
                                                _opt_ptr(tok), stride, _opt_ptr(ln), N, L, U, _opt_ptr(weights),
                                                _opt_ptr(grad_out)))

        def _ctc_lattice_args(self, who, arcs, num_arcs, num_nodes, arc_weights, frames, A, row_stride, max_states):
            """(frames array or None, A, row stride, max_states) of a ctc_lattice_score call"""
            n = len(self)
            if arcs is not None and hasattr(arcs, "data_ptr"):
                t = arcs
                if str(t.dtype) != "torch.int32" or t.dim() != 3 or t.shape[0] != n or t.shape[2] != 3:
                    raise ValueError(f"{who}: arcs must be an int32 tensor [B, A, 3]")
                if t.stride(2) != 1 or (t.shape[1] > 1 and t.stride(1) != 3):
                    raise ValueError(f"{who}: arcs must have contiguous rows of (src, dst, label)")
                rows = t.stride(0) if t.shape[0] > 1 else max(3 * t.shape[1], 1)
                for name, given, have in (("A", A, t.shape[1]), ("row_stride", row_stride, rows)):
                    if given is not None and int(given) != int(have):
                        raise ValueError(f"{who}: {name} = {given} is not what arcs says ({have})")
                A, row_stride = t.shape[1], rows
                if hasattr(t, "is_cuda") and not t.is_cuda:
                    raise ValueError(f"{who}: arcs must be a CUDA tensor")
            if A is None or row_stride is None:
                raise ValueError(f"{who}: a device address needs A and row_stride")
            A = int(A)
            for t, name in ((num_arcs, "num_arcs"), (num_nodes, "num_nodes")):
                if t is not None and hasattr(t, "data_ptr"):
                    if str(t.dtype) != "torch.int32" or not t.is_contiguous() or t.numel() != n:
                        raise ValueError(f"{who}: {name} must be an int32 contiguous tensor [B]")
                    if hasattr(t, "is_cuda") and not t.is_cuda:
                        raise ValueError(f"{who}: {name} must be a CUDA tensor")
            if arc_weights is not None and hasattr(arc_weights, "data_ptr"):
                t = arc_weights
                if str(t.dtype) != "torch.float32" or not t.is_contiguous() or t.numel() != n * A:
                    raise ValueError(f"{who}: arc_weights must be a float32 contiguous tensor [B, A]")
                if hasattr(t, "is_cuda") and not t.is_cuda:
                    raise ValueError(f"{who}: arc_weights must be a CUDA tensor")
            fr, _ = _frames_arg(who, frames, n)
            if max_states is None:
                max_states = max(1, min(2 * A + 1, 4096))  # (a lattice of A arcs that reach its end has <= A + 1 nodes)
            return fr, A, int(row_stride), int(max_states)

        def ctc_lattice_score(self, arcs, num_arcs, num_nodes, scores_out, arc_weights=None, frames=None, blank=0,
                              max_states=None, A=None, row_stride=None):
            """The exact CTC log score of one device-resident acyclic token lattice per utterance under the slabs of a
            Batch.linear, results left on the device (gtnx_batch_ctc_lattice_score; DESIGN section 35 holds the
            contract): scores_out[b] = log sum over the lattice's paths p of exp(w(p) + ctc_score(emissions_b[:T_b],
            labels(p))), every decomposition and every alignment at once, nothing subtracted.  `arcs`: int32 CUDA tensor
            [B, A, 3] of (src, dst, label) rows, 0 <= src < dst < num_nodes, sorted by dst within an utterance, or a
            device address with A and row_stride (elements between utterances, >= 3 A); `num_arcs`, `num_nodes`: int32
            [B] on the device (node 0 starts, the last node accepts); `arc_weights`: float32 [B, A] or None (zeros);
            `scores_out`: float32 [B]; `frames`: T_b per element (0 .. M) or None; `max_states` (1 .. 4096, default
            min(2 A + 1, 4096)): the bound on nodes + arcs that sizes LDS -- larger lattices score -inf, as do invalid
            ones (an arc that is none, a label outside 0 .. C - 1, a weight that is +inf or NaN), ones no alignment
            fits, and T_b == 0.  One launch, no copy back and no wait."""
            fr, A, stride, SM = self._ctc_lattice_args("ctc_lattice_score", arcs, num_arcs, num_nodes, arc_weights,
                                                       frames, A, row_stride, max_states)
            if scores_out is not None and hasattr(scores_out, "data_ptr"):
                if (str(scores_out.dtype) != "torch.float32" or not scores_out.is_contiguous()
                        or scores_out.numel() != len(self)):
                    raise ValueError("ctc_lattice_score: scores_out must be a float32 contiguous tensor [B]")
            check(lib.gtnx_batch_ctc_lattice_score(self._h, fr.ctypes.data if fr is not None else None, int(blank),
                                                   _opt_ptr(arcs), stride, _opt_ptr(num_arcs), _opt_ptr(num_nodes),
                                                   _opt_ptr(arc_weights), A, SM, _opt_ptr(scores_out)))

        def ctc_lattice_score_grad(self, arcs, num_arcs, num_nodes, weights, grad_out, arc_grad_out=None,
                                   arc_weights=None, frames=None, blank=0, max_states=None, A=None, row_stride=None):
            """grad_out[b, t, c] = weights[b] * d score[b] / d emissions[b, t, c] for the scores of `ctc_lattice_score`
            (gtnx_batch_ctc_lattice_score_grad): `weights` float32 [B] on the device, `grad_out` float32 [B, M, C], every
            element written (zeros where nothing lands, rows from T_b on included); `arc_grad_out` float32 [B, A] or None:
            weights[b] * d score[b] / d arc_weights[b, a], weights[b] times the posterior that the arc is used, zeros at
            or past num_arcs[b].  Utterances with a -inf score or a weight of exactly 0 get zeros.  Stateless: the alpha
            rows are recomputed into pooled scratch (sliced beyond 256 MiB, same bits); the sums are taken in a fixed
            order without atomics, so the results have the same bits run to run."""
            who = "ctc_lattice_score_grad"
            fr, A, stride, SM = self._ctc_lattice_args(who, arcs, num_arcs, num_nodes, arc_weights, frames, A,
                                                       row_stride, max_states)
            n = len(self)
            for o, count, what in ((weights, n, "weights must be a float32 contiguous tensor [B]"),
                                   (arc_grad_out, n * A, "arc_grad_out must be a float32 contiguous tensor [B, A]")):
                if o is not None and hasattr(o, "data_ptr"):
                    if str(o.dtype) != "torch.float32" or not o.is_contiguous() or o.numel() != count:
                        raise ValueError(f"{who}: {what}")
            if grad_out is not None and hasattr(grad_out, "data_ptr"):
                m, c = C.c_int(-1), C.c_int(-1)
                check(lib.gtnx_batch_linear_shape(self._h, C.byref(m), C.byref(c)))
                if (str(grad_out.dtype) != "torch.float32" or not grad_out.is_contiguous()
                        or (m.value >= 0 and grad_out.numel() != n * m.value * c.value)):
                    raise ValueError(f"{who}: grad_out must be a float32 contiguous tensor [B, M, C]")
            check(lib.gtnx_batch_ctc_lattice_score_grad(self._h, fr.ctypes.data if fr is not None else None, int(blank),
                                                        _opt_ptr(arcs), stride, _opt_ptr(num_arcs), _opt_ptr(num_nodes),
                                                        _opt_ptr(arc_weights), A, SM, _opt_ptr(weights),
                                                        _opt_ptr(grad_out), _opt_ptr(arc_grad_out)))

        def ctc_lattice_align(self, arcs, num_arcs, num_nodes, scores_out, path_len_out, path_arcs_out,
                              path_tokens_out, starts_out, ends_out, token_scores_out=None, frame_arcs_out=None,
                              arc_weights=None, frames=None, blank=0, max_states=None, A=None, row_stride=None, P=None,
                              out_stride=None, frame_stride=None):
            """The best (lattice path, alignment) pair of one device-resident token lattice per utterance under the
            slabs of a Batch.linear, results left on the device (gtnx_batch_ctc_lattice_align; DESIGN section 38 holds
            the contract).  `arcs`, `num_arcs`, `num_nodes`, `arc_weights`, `frames`, `blank`, `max_states`, A and
            row_stride are those of `ctc_lattice_score`.  `scores_out` float32 [B]: the best w(p) + alignment score, -inf
            without a path; `path_len_out` int32 [B]: the arcs on the best path; `path_arcs_out` / `path_tokens_out` /
            `starts_out` / `ends_out` int32 [B, P]: the arc indices in path order, their labels, the first frame of each
            and one past its last, -1 from path_len on and without a path (a path longer than P keeps its length and
            writes its first P); `token_scores_out` float32 [B, P] or None: the arc's emissions summed in frame order;
            `frame_arcs_out` int32 [B, M] or None: the arc of every frame, -1 on blank frames and from T_b on.  Tensors
            need contiguous, equally spaced rows (views of wider tensors are fine: only the widths P and M are
            written); device addresses go with P, `out_stride` (>= P, default P) and `frame_stride` (>= M, default M).
            Float32 max-plus, of equal candidates the first in the forward's order: the same bits every time.  No copy
            back and no wait."""
            who = "ctc_lattice_align"
            fr, A, stride, SM = self._ctc_lattice_args(who, arcs, num_arcs, num_nodes, arc_weights, frames, A,
                                                       row_stride, max_states)
            n = len(self)

            def rows_of(t, name, dtype, width, given):
                """(width, row stride) of an output: those of a tensor [B, width], else what was given"""
                if t is None or not hasattr(t, "data_ptr"):
                    return width, given
                if str(t.dtype) != dtype or t.dim() != 2 or t.shape[0] != n or (width is not None
                                                                                 and t.shape[1] != width):
                    raise ValueError(f"{who}: {name} must be a {dtype[6:]} tensor [B, {'M' if name == 'frame_arcs_out' else 'P'}]")
                if t.shape[1] > 1 and t.stride(1) != 1:
                    raise ValueError(f"{who}: {name} must have contiguous rows")
                rows = t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)
                if given is not None and int(given) != int(rows):
                    raise ValueError(f"{who}: the outputs must have one row stride ({name} has {rows}, not {given})")
                return t.shape[1], rows
            P = None if P is None else int(P)
            for t, name, dtype in ((path_arcs_out, "path_arcs_out", "torch.int32"),
                                   (path_tokens_out, "path_tokens_out", "torch.int32"),
                                   (starts_out, "starts_out", "torch.int32"), (ends_out, "ends_out", "torch.int32"),
                                   (token_scores_out, "token_scores_out", "torch.float32")):
                P, out_stride = rows_of(t, name, dtype, P, out_stride)
            _, frame_stride = rows_of(frame_arcs_out, "frame_arcs_out", "torch.int32", None, frame_stride)
            if P is None:
                raise ValueError(f"{who}: device addresses need P")
            if out_stride is None:
                out_stride = P
            if frame_stride is None:
                m, c = C.c_int(-1), C.c_int(-1)
                check(lib.gtnx_batch_linear_shape(self._h, C.byref(m), C.byref(c)))
                frame_stride = max(m.value, 0)
            for o, dtype, name in ((scores_out, "torch.float32", "scores_out"), (path_len_out, "torch.int32", "path_len_out")):
                if o is not None and hasattr(o, "data_ptr"):
                    if str(o.dtype) != dtype or not o.is_contiguous() or o.numel() != n:
                        raise ValueError(f"{who}: {name} must be a {dtype[6:]} contiguous tensor [B]")
            check(lib.gtnx_batch_ctc_lattice_align(self._h, fr.ctypes.data if fr is not None else None, int(blank),
                                                   _opt_ptr(arcs), stride, _opt_ptr(num_arcs), _opt_ptr(num_nodes),
                                                   _opt_ptr(arc_weights), A, SM, _opt_ptr(scores_out),
                                                   _opt_ptr(path_len_out), _opt_ptr(path_arcs_out),
                                                   _opt_ptr(path_tokens_out), _opt_ptr(starts_out), _opt_ptr(ends_out),
                                                   _opt_ptr(token_scores_out), int(P), int(out_stride),
                                                   _opt_ptr(frame_arcs_out), int(frame_stride)))

        def _token_align_outputs(self, who, N, L, scores_out, starts_out, ends_out, token_scores_out, frame_tokens_out,
                                 out_stride, frame_stride):
            """What `ctc_token_align` and `asg_token_align` check of their outputs alike.  Returns (out_stride,
            frame_stride), or (None, None) for a call without pairs whose scores are a tensor: nothing to do."""
            n = len(self)

            def rows_of(t, name, dtype, width, given):
                """the row stride of an output: that of a tensor [B, N, width], else `given`"""
                if t is None or not hasattr(t, "data_ptr"):
                    return given
                if str(t.dtype) != dtype or t.dim() != 3 or tuple(t.shape[:2]) != (n, N) or (width is not None
                                                                                               and t.shape[2] != width):
                    raise ValueError(f"{who}: {name} must be a {dtype[6:]} tensor [B, N, {'L' if name != 'frame_tokens_out' else 'M'}]")
                if ((t.shape[2] > 1 and t.stride(2) != 1)
                        or (t.shape[0] > 1 and t.shape[1] > 1 and t.stride(0) != t.shape[1] * t.stride(1))):
                    raise ValueError(f"{who}: {name} must have contiguous rows, equally spaced")
                rows = t.stride(1) if t.shape[1] > 1 else (t.stride(0) if t.shape[0] > 1 else max(t.shape[2], 1))
                if given is not None and int(given) != int(rows):
                    raise ValueError(f"{who}: the outputs must have one row stride ({name} has {rows}, not {given})")
                return rows
            for t, name, dtype in ((starts_out, "starts_out", "torch.int32"), (ends_out, "ends_out", "torch.int32"),
                                   (token_scores_out, "token_scores_out", "torch.float32")):
                out_stride = rows_of(t, name, dtype, L, out_stride)
            frame_stride = rows_of(frame_tokens_out, "frame_tokens_out", "torch.int32", None, frame_stride)
            if out_stride is None:
                out_stride = L
            if frame_stride is None:
                m, c = C.c_int(-1), C.c_int(-1)
                check(lib.gtnx_batch_linear_shape(self._h, C.byref(m), C.byref(c)))
                frame_stride = max(m.value, 0)
            if scores_out is not None and hasattr(scores_out, "data_ptr"):
                if (str(scores_out.dtype) != "torch.float32" or not scores_out.is_contiguous()
                        or scores_out.numel() != n * N):
                    raise ValueError(f"{who}: scores_out must be a float32 contiguous tensor [B, N]")
                if n * N == 0:
                    return None, None
            return int(out_stride), int(frame_stride)

        def ctc_token_align(self, tokens, lengths, scores_out, starts_out, ends_out, token_scores_out=None,
                            frame_tokens_out=None, frames=None, blank=0, max_length=None, N=None, L=None,
                            row_stride=None, out_stride=None, frame_stride=None):
            """The best alignment of all B * N device-resident hypotheses under the slabs of a Batch.linear, results left
            on the device (gtnx_batch_ctc_token_align; DESIGN section 24 holds the contract).  `tokens`, `lengths`,
            `frames`, `blank`, `max_length`, N, L and row_stride are those of `ctc_score`.  `scores_out` float32 [B, N]:
            the Viterbi score, -inf without a path; `starts_out` / `ends_out` int32 [B, N, L]: the first frame of token i
            and one past its last, -1 for i >= len and without a path; `token_scores_out` float32 [B, N, L] or None: the
            token's emissions summed in frame order; `frame_tokens_out` int32 [B, N, M] or None: the token index of every
            frame, -1 on blank frames and from T_b on.  Tensors need contiguous, equally spaced rows (views of wider
            tensors are fine: only the widths L and M are written); device addresses go with `out_stride` (>= L, default
            L) and `frame_stride` (>= M, default M).  Float32 max-plus with the tie rule of `viterbi_align`: the same bits
            every time.  No copy back and no wait."""
            who = "ctc_token_align"
            fr, tok, stride, ln, N, L, U = self._ctc_score_args(who, tokens, lengths, frames, N, L, row_stride, max_length)
            out_stride, frame_stride = self._token_align_outputs(who, N, L, scores_out, starts_out, ends_out,
                                                                 token_scores_out, frame_tokens_out, out_stride,
                                                                 frame_stride)
            if out_stride is None:
                return
            check(lib.gtnx_batch_ctc_token_align(self._h, fr.ctypes.data if fr is not None else None, int(blank),
                                                 _opt_ptr(tok), stride, _opt_ptr(ln), N, L, U, _opt_ptr(scores_out),
                                                 _opt_ptr(starts_out), _opt_ptr(ends_out), _opt_ptr(token_scores_out),
                                                 int(out_stride), _opt_ptr(frame_tokens_out), int(frame_stride)))

        def _asg_score_table(self, who, table):
            """the [C + C * C] table of an asg_score call, checked where it is a tensor"""
            if table is not None and hasattr(table, "data_ptr"):
                if (str(table.dtype) != "torch.float32" or table.dim() != 1 or not table.is_contiguous()
                        or not table.is_cuda):
                    raise ValueError(f"{who}: table must be a float32 contiguous CUDA tensor [C + C * C]")
                m, c = C.c_int(-1), C.c_int(-1)
                check(lib.gtnx_batch_linear_shape(self._h, C.byref(m), C.byref(c)))
                if c.value >= 0 and table.numel() != c.value + c.value * c.value:
                    raise ValueError(f"{who}: table has {table.numel()} entries, {c.value} labels need "
                                     f"{c.value + c.value * c.value}")
            return table

        def asg_score(self, table, tokens, lengths, scores_out, frames=None, max_length=None, N=None, L=None,
                      row_stride=None):
            """The ASG force-align term of all B * N device-resident hypotheses under the slabs of a Batch.linear, results
            left on the device (gtnx_batch_asg_score; DESIGN section 25 holds the contract): scores_out[b, k] =
            forwardScore(emissions_b[:T_b] o (forceAlign(tokens[b, k, :len]) o transitions)) with len = clamp(lengths[b, k],
            0, L), log semiring, nothing subtracted.  `table`: float32 CUDA tensor [C + C * C] or a device address -- entry
            y is start[y], entry C + i * C + j is transitions[i, j], label j followed by label i
            (`torch_loss._asg_weights(start, transitions)`, the table `ctc_beam_decode(lm=...)` takes); `tokens`, `lengths`,
            `frames`, `max_length`, N, L and row_stride are those of `ctc_score` (tokens are labels only: there is no
            blank, equal neighbours are legal).  -inf, never NaN: len == 0, T_b < len, len > max_length, a token inside the
            length outside 0 .. C - 1, no alignment above -inf.  One launch, no copy back and no wait."""
            fr, tok, stride, ln, N, L, U = self._ctc_score_args("asg_score", tokens, lengths, frames, N, L, row_stride,
                                                                max_length)
            table = self._asg_score_table("asg_score", table)
            if scores_out is not None and hasattr(scores_out, "data_ptr"):
                if (str(scores_out.dtype) != "torch.float32" or not scores_out.is_contiguous()
                        or scores_out.numel() != len(self) * N):
                    raise ValueError("asg_score: scores_out must be a float32 contiguous tensor [B, N]")
                if len(self) * N == 0:
                    return
            check(lib.gtnx_batch_asg_score(self._h, fr.ctypes.data if fr is not None else None, _opt_ptr(table),
                                           _opt_ptr(tok), stride, _opt_ptr(ln), N, L, U, _opt_ptr(scores_out)))

        def asg_token_align(self, tokens, lengths, scores_out, starts_out, ends_out, token_scores_out=None,
                            frame_tokens_out=None, frames=None, table=None, max_length=None, N=None, L=None,
                            row_stride=None, out_stride=None, frame_stride=None):
            """The best ASG alignment of all B * N device-resident hypotheses under the slabs of a Batch.linear, results
            left on the device (gtnx_batch_asg_token_align; DESIGN section 28 holds the contract).  `table`, `tokens`,
            `lengths`, `frames`, `max_length`, N, L and row_stride are those of `asg_score`; the outputs, `out_stride` and
            `frame_stride` are those of `ctc_token_align`, except that `frame_tokens_out` is never -1 inside a path (ASG
            has no blank).  A pair has no path (-inf, rows of -1) exactly where `asg_score` gives -inf.  Float32 max-plus
            with the arithmetic of `asg_forced_align`, of two equal candidates the step: the same bits every time, and
            its scores where both apply.  No copy back and no wait."""
            who = "asg_token_align"
            fr, tok, stride, ln, N, L, U = self._ctc_score_args(who, tokens, lengths, frames, N, L, row_stride, max_length)
            table = self._asg_score_table(who, table)
            out_stride, frame_stride = self._token_align_outputs(who, N, L, scores_out, starts_out, ends_out,
                                                                 token_scores_out, frame_tokens_out, out_stride,
                                                                 frame_stride)
            if out_stride is None:
                return
            check(lib.gtnx_batch_asg_token_align(self._h, fr.ctypes.data if fr is not None else None, _opt_ptr(table),
                                                 _opt_ptr(tok), stride, _opt_ptr(ln), N, L, U, _opt_ptr(scores_out),
                                                 _opt_ptr(starts_out), _opt_ptr(ends_out), _opt_ptr(token_scores_out),
                                                 int(out_stride), _opt_ptr(frame_tokens_out), int(frame_stride)))

        def asg_score_grad(self, table, tokens, lengths, weights, grad_out=None, grad_table_out=None, frames=None,
                           max_length=None, N=None, L=None, row_stride=None):
            """The gradients of the scores of `asg_score` under `weights` (float32 [B, N] on the device), in one stateless
            call (gtnx_batch_asg_score_grad): `grad_out` (float32 [B, M, C] or None) = sum over k of weights[b, k] * d
            score[b, k] / d emissions[b], every element written (zeros where nothing lands, rows from T_b on included);
            `grad_table_out` (float32 [C + C * C] or None) = sum over all pairs of weights * d score / d table, every
            entry written; not both None.  A call without pairs (B * N == 0) writes nothing.  Pairs with a -inf score or a
            weight of exactly 0 add nothing.  The alpha rows are recomputed into pooled scratch (sliced beyond 256 MiB,
            same bits); the sums are taken in a fixed order without atomics, so both results have the same bits run to
            run."""
            fr, tok, stride, ln, N, L, U = self._ctc_score_args("asg_score_grad", tokens, lengths, frames, N, L,
                                                                row_stride, max_length)
            table = self._asg_score_table("asg_score_grad", table)
            if grad_out is None and grad_table_out is None:
                raise ValueError("asg_score_grad: neither grad_out nor grad_table_out given")
            for o, what in ((weights, "weights must be a float32 contiguous tensor [B, N]"),
                            (grad_out, "grad_out must be a float32 contiguous tensor [B, M, C]"),
                            (grad_table_out, "grad_table_out must be a float32 contiguous tensor [C + C * C]")):
                if o is not None and hasattr(o, "data_ptr"):
                    if str(o.dtype) != "torch.float32" or not o.is_contiguous():
                        raise ValueError(f"asg_score_grad: {what}")
            if weights is not None and hasattr(weights, "data_ptr") and weights.numel() != len(self) * N:
                raise ValueError("asg_score_grad: weights must be a float32 contiguous tensor [B, N]")
            m, c = C.c_int(-1), C.c_int(-1)
            check(lib.gtnx_batch_linear_shape(self._h, C.byref(m), C.byref(c)))
            if grad_out is not None and hasattr(grad_out, "data_ptr"):
                if m.value >= 0 and grad_out.numel() != len(self) * m.value * c.value:
                    raise ValueError("asg_score_grad: grad_out must be a float32 contiguous tensor [B, M, C]")
            if grad_table_out is not None and hasattr(grad_table_out, "data_ptr"):
                if c.value >= 0 and grad_table_out.numel() != c.value + c.value * c.value:
                    raise ValueError("asg_score_grad: grad_table_out must be a float32 contiguous tensor [C + C * C]")
            if len(self) * N == 0 and any(hasattr(o, "data_ptr") for o in (grad_out, grad_table_out)):
                return
            check(lib.gtnx_batch_asg_score_grad(self._h, fr.ctypes.data if fr is not None else None, _opt_ptr(table),
                                                _opt_ptr(tok), stride, _opt_ptr(ln), N, L, U, _opt_ptr(weights),
                                                _opt_ptr(grad_out), _opt_ptr(grad_table_out)))

        def asg_lattice_score(self, table, arcs, num_arcs, num_nodes, scores_out, arc_weights=None, frames=None,
                              max_states=None, max_edges=None, A=None, row_stride=None):
            """The exact ASG log score of one device-resident acyclic token lattice per utterance under the slabs of a
            Batch.linear, results left on the device (gtnx_batch_asg_lattice_score; DESIGN section 37 holds the contract):
            scores_out[b] = log sum over the lattice's paths p of exp(w(p) + asg_score(emissions_b[:T_b], table,
            labels(p))), nothing subtracted.  `table` is that of `asg_score`; `arcs`, `num_arcs`, `num_nodes`,
            `arc_weights`, `frames`, `max_states`, A and row_stride are those of `ctc_lattice_score` (the states are the
            arcs: there is no blank, equal neighbours are legal).  `max_edges` (1 .. 2^21, default min(8 * max_states,
            2^21)): the caller's bound on the sum over the arcs of the in-degree of their src.  -inf, never NaN: T_b == 0,
            num_nodes < 1, nodes + arcs > max_states, more edges than max_edges, an invalid arc or weight, no alignment
            (a one-node lattice has none).  One launch, no copy back and no wait."""
            who = "asg_lattice_score"
            fr, A, stride, SM = self._ctc_lattice_args(who, arcs, num_arcs, num_nodes, arc_weights, frames, A, row_stride,
                                                       max_states)
            table = self._asg_score_table(who, table)
            if max_edges is None:
                max_edges = min(8 * SM, 1 << 21)
            if scores_out is not None and hasattr(scores_out, "data_ptr"):
                if (str(scores_out.dtype) != "torch.float32" or not scores_out.is_contiguous()
                        or scores_out.numel() != len(self)):
                    raise ValueError(f"{who}: scores_out must be a float32 contiguous tensor [B]")
            check(lib.gtnx_batch_asg_lattice_score(self._h, fr.ctypes.data if fr is not None else None, _opt_ptr(table),
                                                   _opt_ptr(arcs), stride, _opt_ptr(num_arcs), _opt_ptr(num_nodes),
                                                   _opt_ptr(arc_weights), A, SM, int(max_edges), _opt_ptr(scores_out)))

        def asg_lattice_score_grad(self, table, arcs, num_arcs, num_nodes, weights, grad_out=None, grad_table_out=None,
                                   arc_grad_out=None, arc_weights=None, frames=None, max_states=None, max_edges=None,
                                   A=None, row_stride=None):
            """The gradients of the scores of `asg_lattice_score` under `weights` (float32 [B] on the device), in one
            stateless call (gtnx_batch_asg_lattice_score_grad): `grad_out` (float32 [B, M, C] or None) = weights[b] * d
            score[b] / d emissions[b]; `grad_table_out` (float32 [C + C * C] or None) = sum over b of weights[b] * d
            score[b] / d table; `arc_grad_out` (float32 [B, A] or None) = weights[b] * the posterior of every arc, zeros
            at or past num_arcs[b]; not all three None, and every element of a given output is written.  Utterances with
            a -inf score or a weight of exactly 0 add nothing.  Alpha rows and one cell per edge are recomputed into
            pooled scratch (sliced beyond 256 MiB, same bits); the sums are taken in a fixed order without atomics, so
            the results have the same bits run to run."""
            who = "asg_lattice_score_grad"
            fr, A, stride, SM = self._ctc_lattice_args(who, arcs, num_arcs, num_nodes, arc_weights, frames, A, row_stride,
                                                       max_states)
            table = self._asg_score_table(who, table)
            if max_edges is None:
                max_edges = min(8 * SM, 1 << 21)
            if grad_out is None and grad_table_out is None and arc_grad_out is None:
                raise ValueError(f"{who}: none of grad_out, grad_table_out and arc_grad_out given")
            n = len(self)
            m, c = C.c_int(-1), C.c_int(-1)
            check(lib.gtnx_batch_linear_shape(self._h, C.byref(m), C.byref(c)))
            known = m.value >= 0
            for o, count, what in ((weights, n, "weights must be a float32 contiguous tensor [B]"),
                                   (grad_out, n * m.value * c.value if known else None,
                                    "grad_out must be a float32 contiguous tensor [B, M, C]"),
                                   (grad_table_out, c.value + c.value * c.value if known else None,
                                    "grad_table_out must be a float32 contiguous tensor [C + C * C]"),
                                   (arc_grad_out, n * A, "arc_grad_out must be a float32 contiguous tensor [B, A]")):
                if o is not None and hasattr(o, "data_ptr"):
                    if (str(o.dtype) != "torch.float32" or not o.is_contiguous()
                            or (count is not None and o.numel() != count)):
                        raise ValueError(f"{who}: {what}")
            check(lib.gtnx_batch_asg_lattice_score_grad(self._h, fr.ctypes.data if fr is not None else None,
                                                        _opt_ptr(table), _opt_ptr(arcs), stride, _opt_ptr(num_arcs),
                                                        _opt_ptr(num_nodes), _opt_ptr(arc_weights), A, SM, int(max_edges),
                                                        _opt_ptr(weights), _opt_ptr(grad_out), _opt_ptr(grad_table_out),
                                                        _opt_ptr(arc_grad_out)))

    ns.Batch = Batch

    def _batch_fn(cfn, *args):
        h = C.c_void_p()
        check(cfn(*[a._h for a in args], C.byref(h)))
        return Batch._from_handle(h.value)

    def _with_batches(plain, cfn):
        def f(*args, **kw):
            if args and all(isinstance(a, Batch) for a in args) and not kw:
                return _batch_fn(cfn, *args)
            return plain(*args, **kw)
        f.__doc__ = plain.__doc__
        f.__name__ = getattr(plain, "__name__", "f")
        return f

    if hasattr(lib, "gtnx_batch_negate"):  # (not in the reference-backed shim the CPU tests load)
        for _name in ("negate", "add", "subtract", "compose", "intersect", "forward_score", "viterbi_score",
                      "viterbi_path"):
            setattr(ns, _name, _with_batches(getattr(ns, _name), getattr(lib, "gtnx_batch_" + _name)))

    def subtract_into(a, b, items_device):
        """subtract(a, b) of two batches with the values written straight into `items_device` (a torch CUDA tensor or
        a device address, borrowed: it must outlive the result) -- gtnx_batch_subtract_into"""
        h = C.c_void_p()
        check(lib.gtnx_batch_subtract_into(a._h, b._h, _as_dev_ptr(items_device), C.byref(h)))
        r = Batch._from_handle(h.value)
        r._keep = items_device
        return r

    if hasattr(lib, "gtnx_batch_subtract_into"):
        ns.subtract_into = subtract_into

    _plain_backward = ns.backward

    def backward(g, grad_or_retain=None, retain_graph=False):
        if isinstance(g, Batch):
            r = grad_or_retain if isinstance(grad_or_retain, bool) else retain_graph
            check(lib.gtnx_batch_backward(g._h, int(bool(r))))
            return
        return _plain_backward(g, grad_or_retain, retain_graph)

    ns.backward = backward

    def parallel_for(fn, iterable):
        """gtn.parallel_for (_parallel.cpp:20-26).  The device engine batches
        through list arguments instead; this runs the callable serially."""
        for i in iterable:
            fn(i)

    ns.parallel_for = parallel_for

    # ---------------------------------------------------------------- runtime
    def backend():
        return lib.gtnx_backend().decode()

    def device_count():
        return lib.gtnx_device_count()

    def synchronize():
        check(lib.gtnx_synchronize())

    def set_device(i):
        check(lib.gtnx_set_device(int(i)))

    def set_stream(stream):
        """stream: hipStream_t address (torch.cuda.Stream.cuda_stream) or None"""
        check(lib.gtnx_set_stream(int(stream) if stream else None))

    def compose_mode(mode):
        """0: build compositions; 1: keep chain compositions symbolic whenever eligible; 2: when the
        per-utterance sweep kernels apply; -1 (the default): as 2 for partners built on the host, else 0.
        Returns the previous mode (gtn_amd.h)."""
        prev = C.c_int()
        check(lib.gtnx_compose_mode(int(mode), C.byref(prev)))
        return prev.value

    def memory_stats():
        r, u = C.c_uint64(), C.c_uint64()
        check(lib.gtnx_memory_stats(C.byref(r), C.byref(u)))
        return {"reserved": r.value, "in_use": u.value}

    def prof_enable(on=True):
        check(lib.gtnx_prof_enable(int(bool(on))))

    def prof_reset():
        check(lib.gtnx_prof_reset())

    def prof_get(name):
        ms, n, b = C.c_double(), C.c_int64(), C.c_double()
        check(lib.gtnx_prof_get(name.encode(), C.byref(ms), C.byref(n), C.byref(b)))
        return {"total_ms": ms.value, "launches": n.value, "algorithmic_bytes": b.value}

    def prof_names():
        buf = C.create_string_buffer(4096)
        check(lib.gtnx_prof_names(buf, 4096))
        return [s for s in buf.value.decode().split("\n") if s]

    def debug_symbolic_route(g, tropical=False):
        """which kernel family scores this symbolic product (gtn_amd/csrc/ops_symbolic.cpp); None if `g` is built"""
        r = C.c_int(-1)
        check(lib.gtnx_debug_symbolic_route(g._h, int(bool(tropical)), C.byref(r)))
        if r.value < 0:
            return None
        buf = C.create_string_buffer(32)
        check(lib.gtnx_debug_route_name(r.value, buf, 32))
        return buf.value.decode()

    def debug_viterbi_ties():
        """(seen, unresolved): best paths of symbolic dense-partner products that ran through an exact tie / of those,
        the ones whose product was too large to rebuild and replay the reference's queue on (include/gtn_amd.h)"""
        return _stats2(lib.gtnx_debug_viterbi_ties)

    def debug_shortest_routes():
        """{cell name: launches since the process started} of the built-graph shortest-distance kernels
        (gtn_amd/csrc/shortest.hip; include/gtn_amd.h: gtnx_debug_shortest_routes).  Needs no GPU."""
        n = C.c_int(0)
        check(lib.gtnx_debug_shortest_routes(-1, None, 0, None, C.byref(n)))
        out = {}
        for cell in range(n.value):
            buf = C.create_string_buffer(48)
            cnt = C.c_int64(0)
            check(lib.gtnx_debug_shortest_routes(cell, buf, 48, C.byref(cnt), None))
            out[buf.value.decode()] = int(cnt.value)
        return out

    def debug_compose_routes():
        """{cell name: products since the process started} of compose / intersect: first kernel, hand-backs, bitmap
        layout and the finished product's attributes (gtn_amd/csrc/ops_compose.cpp; include/gtn_amd.h:
        gtnx_debug_compose_routes).  Needs no GPU."""
        n = C.c_int(0)
        check(lib.gtnx_debug_compose_routes(-1, None, 0, None, C.byref(n)))
        out = {}
        for cell in range(n.value):
            buf = C.create_string_buffer(48)
            cnt = C.c_int64(0)
            check(lib.gtnx_debug_compose_routes(cell, buf, 48, C.byref(cnt), None))
            out[buf.value.decode()] = int(cnt.value)
        return out

    def debug_align_stats():
        """(fast, fallback): utterances Batch.viterbi_align has aligned so far by its one launch / through the path
        graphs of viterbi_path (include/gtn_amd.h: gtnx_batch_align_stats)"""
        return _stats2(lib.gtnx_batch_align_stats)

    def debug_decode_stats():
        """(fast, fallback): utterances Batch.viterbi_decode has decoded so far by its one launch / through the path
        graphs of viterbi_path (include/gtn_amd.h: gtnx_batch_decode_stats)"""
        return _stats2(lib.gtnx_batch_decode_stats)

    def debug_linear_decode_stats():
        """(fast, fallback): utterances Batch.linear_decode has decoded so far by its two launches / through the path
        graphs of viterbi_path (include/gtn_amd.h: gtnx_batch_linear_decode_stats)"""
        return _stats2(lib.gtnx_batch_linear_decode_stats)

    def debug_ctc_beam_stats():
        """(calls, utterances): calls of Batch.ctc_beam_decode that have launched so far and the utterances they
        decoded (include/gtn_amd.h: gtnx_batch_ctc_beam_stats)"""
        return _stats2(lib.gtnx_batch_ctc_beam_stats)

    def debug_ctc_sample_stats():
        """(calls, utterances): calls of Batch.ctc_sample that have launched so far and the utterances they sampled
        (include/gtn_amd.h: gtnx_batch_ctc_sample_stats)"""
        return _stats2(lib.gtnx_batch_ctc_sample_stats)

    def debug_asg_sample_stats():
        """(calls, utterances): calls of Batch.asg_sample that have launched so far and the utterances they sampled
        (include/gtn_amd.h: gtnx_batch_asg_sample_stats)"""
        return _stats2(lib.gtnx_batch_asg_sample_stats)

    def debug_ctc_score_stats():
        """(calls, pairs): calls of Batch.ctc_score / Batch.ctc_score_grad that have launched so far and the pairs they
        took (include/gtn_amd.h: gtnx_batch_ctc_score_stats)"""
        return _stats2(lib.gtnx_batch_ctc_score_stats)

    def debug_ctc_token_align_stats():
        """(calls, pairs): calls of Batch.ctc_token_align that have launched so far and the pairs they aligned
        (include/gtn_amd.h: gtnx_batch_ctc_token_align_stats)"""
        return _stats2(lib.gtnx_batch_ctc_token_align_stats)

    def debug_asg_score_stats():
        """(calls, pairs): calls of Batch.asg_score / Batch.asg_score_grad that have launched so far and the pairs they
        took (include/gtn_amd.h: gtnx_batch_asg_score_stats)"""
        return _stats2(lib.gtnx_batch_asg_score_stats)

    def debug_asg_token_align_stats():
        """(calls, pairs): calls of Batch.asg_token_align that have launched so far and the pairs they aligned
        (include/gtn_amd.h: gtnx_batch_asg_token_align_stats)"""
        return _stats2(lib.gtnx_batch_asg_token_align_stats)

    def debug_asg_beam_stats():
        """(calls, utterances): calls of Batch.asg_beam_decode that have launched so far and the utterances they decoded
        (include/gtn_amd.h: gtnx_batch_asg_beam_stats)"""
        return _stats2(lib.gtnx_batch_asg_beam_stats)

    def debug_edit_distance_stats():
        """(calls, pairs): calls of edit_distance that have launched so far and the pairs they computed
        (include/gtn_amd.h: gtnx_batch_edit_distance_stats)"""
        return _stats2(lib.gtnx_batch_edit_distance_stats)

    def edit_distance(hyp, hyp_lengths, ref, ref_lengths, dist_out, ops_out=None, B=None, N=None, L=None, U=None,
                      hyp_stride=None, ref_stride=None):
        """Levenshtein distance (unit costs) of all B * N pairs (hyp[b, k], ref[b]) of token rows on the device, results
        left on the device (gtnx_batch_edit_distance; DESIGN section 21 holds the contract).  `hyp`: int32 CUDA tensor
        [B, N, L] or [B, L] (then N = 1) with contiguous, equally spaced rows, or a device address with B, N, L and
        hyp_stride (elements between rows, >= L); `hyp_lengths`: int32 [B, N], contiguous; `ref`: int32 [B, U] with
        contiguous rows, or an address with U and ref_stride; `ref_lengths`: int32 [B].  The lengths stay on the device:
        the kernel clamps them to 0 .. L / 0 .. U and reads nothing at or past them; tokens are compared with == only.
        `dist_out`: int32 [B, N]; `ops_out`: int32 [B, N, 3] = (substitutions, deletions, insertions) of the walk back
        that prefers the diagonal, then up (a deletion: a reference token without counterpart), then left (an
        insertion), or None: then nothing is kept for the walk and the call is one launch.  L <= 65536, U <= 4096.  No
        copy back and no wait."""
        dims = {"B": B, "N": N, "L": L, "U": U}

        def settle(name, value):
            if dims[name] is not None and int(dims[name]) != int(value):
                raise ValueError(f"edit_distance: {name} = {dims[name]} is not what the tensors say ({value})")
            dims[name] = int(value)

        tensors = []
        if hasattr(hyp, "data_ptr"):
            if str(hyp.dtype) != "torch.int32" or hyp.dim() not in (2, 3):
                raise ValueError("edit_distance: hyp must be an int32 tensor [B, N, L] or [B, L]")
            h = hyp if hyp.dim() == 3 else hyp.unsqueeze(1)
            settle("B", h.shape[0]), settle("N", h.shape[1]), settle("L", h.shape[2])
            rows = h.stride(1) if h.shape[1] > 1 else (h.stride(0) if h.shape[0] > 1 else max(h.shape[2], 1))
            if ((h.shape[2] > 1 and h.stride(2) != 1)
                    or (h.shape[0] > 1 and h.shape[1] > 1 and h.stride(0) != h.shape[1] * h.stride(1))):
                raise ValueError("edit_distance: hyp must have contiguous rows, equally spaced")
            if hyp_stride is not None and int(hyp_stride) != rows:
                raise ValueError("edit_distance: hyp_stride is not the row stride of hyp")
            hyp_stride = rows
            tensors.append(("hyp", hyp))
        if hasattr(ref, "data_ptr"):
            if str(ref.dtype) != "torch.int32" or ref.dim() != 2:
                raise ValueError("edit_distance: ref must be an int32 tensor [B, U]")
            settle("B", ref.shape[0]), settle("U", ref.shape[1])
            rows = ref.stride(0) if ref.shape[0] > 1 else max(ref.shape[1], 1)
            if ref.shape[1] > 1 and ref.stride(1) != 1:
                raise ValueError("edit_distance: ref must have contiguous rows")
            if ref_stride is not None and int(ref_stride) != rows:
                raise ValueError("edit_distance: ref_stride is not the row stride of ref")
            ref_stride = rows
            tensors.append(("ref", ref))
        for name in ("B", "N", "L", "U"):
            if dims[name] is None:
                raise ValueError(f"edit_distance: a device address needs {name}")
        if hyp_stride is None or ref_stride is None:
            raise ValueError("edit_distance: a device address needs hyp_stride / ref_stride")
        b, n, l, u = (dims[k] for k in ("B", "N", "L", "U"))
        for o, count, what in ((hyp_lengths, b * n, "hyp_lengths must be an int32 contiguous tensor [B, N]"),
                               (ref_lengths, b, "ref_lengths must be an int32 contiguous tensor [B]"),
                               (dist_out, b * n, "dist_out must be an int32 contiguous tensor [B, N]"),
                               (ops_out, 3 * b * n, "ops_out must be an int32 contiguous tensor [B, N, 3]")):
            if o is not None and hasattr(o, "data_ptr"):
                if str(o.dtype) != "torch.int32" or not o.is_contiguous() or o.numel() != count:
                    raise ValueError(f"edit_distance: {what}")
                tensors.append((what.split()[0], o))
        for name, t in tensors:  # (a host tensor's address means nothing to the kernel)
            if hasattr(t, "is_cuda") and not t.is_cuda:
                raise ValueError(f"edit_distance: {name} must be a CUDA tensor")

        if b * n == 0 and tensors:
            return  # (no pair, nothing to launch -- and an empty tensor has no address to hand to the engine)

        check(lib.gtnx_batch_edit_distance(_opt_ptr(hyp), int(hyp_stride), _opt_ptr(hyp_lengths), _opt_ptr(ref),
                                           int(ref_stride), _opt_ptr(ref_lengths), b, n, l, u, _opt_ptr(dist_out),
                                           _opt_ptr(ops_out)))

    def debug_ctc_lattice_score_stats():
        """(calls, utterances): calls of Batch.ctc_lattice_score / Batch.ctc_lattice_score_grad that have launched so
        far and the utterances they took (include/gtn_amd.h: gtnx_batch_ctc_lattice_score_stats)"""
        return _stats2(lib.gtnx_batch_ctc_lattice_score_stats)

    def debug_ctc_lattice_align_stats():
        """(calls, utterances): calls of Batch.ctc_lattice_align that have launched so far and the utterances they took
        (include/gtn_amd.h: gtnx_batch_ctc_lattice_align_stats)"""
        return _stats2(lib.gtnx_batch_ctc_lattice_align_stats)

    def debug_asg_lattice_score_stats():
        """(calls, utterances): calls of Batch.asg_lattice_score / Batch.asg_lattice_score_grad that have launched so
        far and the utterances they took (include/gtn_amd.h: gtnx_batch_asg_lattice_score_stats)"""
        return _stats2(lib.gtnx_batch_asg_lattice_score_stats)

    def debug_full_connect_stats():
        """(fast, fallback): utterances whose ASG full-connect score forward_score(compose(Batch.linear(rows=...),
        transitions)) came from the one launch of asg_full.hip / utterances of such a padded batch that took the composed
        elements instead (include/gtn_amd.h: gtnx_batch_full_connect_stats)"""
        return _stats2(lib.gtnx_batch_full_connect_stats)

    if hasattr(lib, "gtnx_batch_align_stats"):
        ns.debug_align_stats = debug_align_stats
    ns.debug_full_connect_stats = debug_full_connect_stats
    ns.debug_decode_stats = debug_decode_stats
    ns.debug_linear_decode_stats = debug_linear_decode_stats
    ns.debug_ctc_beam_stats = debug_ctc_beam_stats
    ns.debug_ctc_sample_stats = debug_ctc_sample_stats
    ns.debug_edit_distance_stats = debug_edit_distance_stats
    ns.debug_ctc_score_stats = debug_ctc_score_stats
    ns.debug_ctc_token_align_stats = debug_ctc_token_align_stats
    ns.debug_ctc_lattice_score_stats = debug_ctc_lattice_score_stats
    ns.debug_ctc_lattice_align_stats = debug_ctc_lattice_align_stats
    ns.debug_asg_score_stats = debug_asg_score_stats
    ns.debug_asg_lattice_score_stats = debug_asg_lattice_score_stats
    ns.debug_asg_token_align_stats = debug_asg_token_align_stats
    ns.debug_asg_beam_stats = debug_asg_beam_stats
    ns.debug_asg_sample_stats = debug_asg_sample_stats
    ns.edit_distance = edit_distance
    ns.debug_symbolic_route = debug_symbolic_route
    ns.debug_viterbi_ties = debug_viterbi_ties
    if hasattr(lib, "gtnx_debug_shortest_routes"):  # (the engine's kernels: not in the reference-backed shim)
        ns.debug_shortest_routes = debug_shortest_routes
    if hasattr(lib, "gtnx_debug_compose_routes"):
        ns.debug_compose_routes = debug_compose_routes

    def debug_tie_ranks(g):
        """(queue_rank, creation_rank) of a CTC-shaped target's nodes, or None (gtn_amd.h: gtnx_debug_tie_ranks)"""
        n = g.num_nodes()
        k, c = np.zeros(n, np.int32), np.zeros(n, np.int32)
        ok = C.c_int()
        check(lib.gtnx_debug_tie_ranks(g._h, k.ctypes.data, c.ctypes.data, C.byref(ok)))
        return (k.tolist(), c.tolist()) if ok.value else None

    ns.debug_tie_ranks = debug_tie_ranks
    ns.backend = backend
    ns.device_count = device_count
    ns.synchronize = synchronize
    ns.set_device = set_device
    ns.set_stream = set_stream
    ns.compose_mode = compose_mode
    ns.memory_stats = memory_stats
    ns.empty_cache = lambda: check(lib.gtnx_empty_cache())
    ns.prof_enable = prof_enable
    ns.prof_reset = prof_reset
    ns.prof_get = prof_get
    ns.prof_names = prof_names
    return ns


def load_txt(api, text):
    """gtn.loadTxt (gtn/utils.cpp:283-345) for the text fixtures of the tests:
    line 1 start nodes, line 2 accept nodes, then `src dst ilabel [olabel [w]]`."""
    lines = [l for l in text.strip("\n").split("\n")]
    starts = [int(x) for x in lines[0].split()]
    accepts = [int(x) for x in lines[1].split()]
    arcs = []
    nmax = max(starts + accepts + [-1])
    for l in lines[2:]:
        f = l.split()
        if not f:
            continue
        s, d, il = int(f[0]), int(f[1]), int(f[2])
        ol = int(f[3]) if len(f) > 3 else il
        w = float(f[4]) if len(f) > 4 else 0.0
        arcs.append((s, d, il, ol, w))
        nmax = max(nmax, s, d)
    g = api.Graph()
    for n in range(nmax + 1):
        g.add_node(n in starts, n in accepts)
    for s, d, il, ol, w in arcs:
        g.add_arc(s, d, il, ol, w)
    return g
