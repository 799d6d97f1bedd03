"""Stream capture through ctypes on the HIP runtime the process already has loaded (torch's): begin a capture in GLOBAL mode —
the strictest: while it is open, a synchronising or allocating HIP call made by ANY thread invalidates it —, end it, look at the
graph (nodes, their types, edges), instantiate, launch, destroy.  Nothing else.

The runtime's path is read from /proc/self/maps after `import torch`; no second copy is loaded.  No environment variable is
set and the number of hardware queues is left alone.  capture() creates no torch tensor between begin and end (the caching
allocator would allocate under capture), always ends the capture in a `finally`, and RETURNS the status of a refused or
invalidated capture together with whatever the captured function raised: nothing is raised from inside the capture region.

A plain module: no fixtures, no pytest."""
import ctypes as C

HIP_SUCCESS = 0
CAPTURE_MODE_GLOBAL = 0          # hipStreamCaptureModeGlobal
NODE_KERNEL, NODE_MEMCPY, NODE_MEMSET = 0, 1, 2
NODE_NAMES = {0: "kernel", 1: "memcpy", 2: "memset", 3: "host", 4: "graph", 5: "empty", 6: "wait_event", 7: "event_record",
              8: "ext_semaphore_signal", 9: "ext_semaphore_wait", 10: "mem_alloc", 11: "mem_free", 12: "memcpy_from_symbol",
              13: "memcpy_to_symbol"}

_hip = None


def runtime_path():
    """the libamdhip64 this process has mapped (import torch first)"""
    with open("/proc/self/maps") as f:
        for line in f:
            path = line.split(None, 5)[-1].strip()
            if "libamdhip64.so" in path and path.startswith("/"):
                return path
    raise RuntimeError("no libamdhip64 is mapped into this process: import torch (or load libspfe.so) first")


def hip():
    global _hip
    if _hip is None:
        L = C.CDLL(runtime_path())           # the path is the loaded copy's: dlopen returns that handle, nothing new is loaded
        vp, pvp, psz = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)
        for name, args in (("hipStreamBeginCapture", [vp, C.c_int]), ("hipStreamEndCapture", [vp, pvp]),
                           ("hipGraphGetNodes", [vp, pvp, psz]), ("hipGraphNodeGetType", [vp, C.POINTER(C.c_int)]),
                           ("hipGraphGetEdges", [vp, pvp, pvp, psz]),
                           ("hipGraphInstantiate", [pvp, vp, pvp, C.c_char_p, C.c_size_t]), ("hipGraphLaunch", [vp, vp]),
                           ("hipGraphExecDestroy", [vp]), ("hipGraphDestroy", [vp]), ("hipGetLastError", [])):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = C.c_int, args
        L.hipGetErrorName.restype, L.hipGetErrorName.argtypes = C.c_char_p, [C.c_int]
        _hip = L
    return _hip


def error_name(status):
    return "hipSuccess" if status == 0 else "%s (%d)" % (hip().hipGetErrorName(int(status)).decode(), status)


class Captured:
    """status: 0, or the HIP status that refused / invalidated the capture (begin's or end's); error: what the captured function
    raised (None: nothing); graph: the hipGraph_t (None when there is none)"""

    def __init__(self, status, error, graph):
        self.status, self.error, self.graph = status, error, graph
        self.exec = None

    @property
    def ok(self):
        return self.status == HIP_SUCCESS and self.error is None and self.graph is not None

    def why(self):
        return "%s%s" % (error_name(self.status), "" if self.error is None else "; the call raised %s" % (self.error,))

    def nodes(self):
        """-> list of (node handle, type)"""
        n = C.c_size_t(0)
        assert hip().hipGraphGetNodes(self.graph, None, C.byref(n)) == 0
        arr = (C.c_void_p * max(n.value, 1))()
        assert hip().hipGraphGetNodes(self.graph, arr, C.byref(n)) == 0
        out = []
        for i in range(n.value):
            t = C.c_int(-1)
            assert hip().hipGraphNodeGetType(arr[i], C.byref(t)) == 0
            out.append((arr[i], t.value))
        return out

    def edges(self):
        """-> list of (from handle, to handle)"""
        n = C.c_size_t(0)
        assert hip().hipGraphGetEdges(self.graph, None, None, C.byref(n)) == 0
        a, b = (C.c_void_p * max(n.value, 1))(), (C.c_void_p * max(n.value, 1))()
        if n.value:
            assert hip().hipGraphGetEdges(self.graph, a, b, C.byref(n)) == 0
        return [(a[i], b[i]) for i in range(n.value)]

    def shape(self):
        """-> dict(kernel, memset, other (names of any other node type), nodes, edges, roots)"""
        nodes, edges = self.nodes(), self.edges()
        has_parent = {t for _, t in edges}
        return dict(kernel=sum(t == NODE_KERNEL for _, t in nodes), memset=sum(t == NODE_MEMSET for _, t in nodes),
                    other=sorted(NODE_NAMES.get(t, str(t)) for _, t in nodes if t not in (NODE_KERNEL, NODE_MEMSET)),
                    nodes=len(nodes), edges=len(edges), roots=sum(h not in has_parent for h, _ in nodes))

    def instantiate(self):
        e = C.c_void_p()
        status = hip().hipGraphInstantiate(C.byref(e), self.graph, None, None, 0)
        if status == 0:
            self.exec = e
        return status

    def launch(self, stream):
        return hip().hipGraphLaunch(self.exec, C.c_void_p(stream))

    def destroy(self):
        if self.exec is not None:
            hip().hipGraphExecDestroy(self.exec)
            self.exec = None
        if self.graph is not None:
            hip().hipGraphDestroy(self.graph)
            self.graph = None


def capture(stream, fn):
    """Capture what fn() enqueues on `stream` (a torch.cuda.Stream) in global mode -> Captured.  fn must create no tensor."""
    L = hip()
    handle = C.c_void_p(stream.cuda_stream)
    status = L.hipStreamBeginCapture(handle, CAPTURE_MODE_GLOBAL)
    if status != 0:
        L.hipGetLastError()
        return Captured(status, None, None)
    error, graph = None, C.c_void_p()
    try:
        fn()
    except Exception as e:              # returned, not raised: the capture is ended first
        error = "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:300] if str(e) else "")
    finally:
        status = L.hipStreamEndCapture(handle, C.byref(graph))
        if status != 0:
            L.hipGetLastError()         # the sticky status of an invalidated capture is this capture's, not the next call's
    return Captured(status, error, graph if status == 0 and graph.value else None)
