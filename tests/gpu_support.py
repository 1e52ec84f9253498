"""Device-side props of the GPU tests: the body of the modules' `torch` fixtures, unrelated work to keep a stream busy,
and a single-process matched transport for the time shards' halo.  Imported by basename like pdw_cases."""
import ctypes as C

_hip = None


def cuda_torch():
    """torch with device 0 current: what the module-scoped `torch` fixtures return."""
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


class Busy:
    """A few tens of milliseconds of unrelated work queued on a stream (large device copies), so that everything
    enqueued behind it is issued with the host ahead of the device."""

    def __init__(self, torch):
        self.torch = torch
        self.src = torch.empty(1 << 30, dtype=torch.float32, device="cuda")   # 4 GiB
        self.dst = torch.empty_like(self.src)
        self.src.zero_()
        torch.cuda.synchronize()

    def queue(self, stream, copies=8):
        with self.torch.cuda.stream(stream):
            for _ in range(copies):
                self.dst.copy_(self.src, non_blocking=True)


def hip_memcpy_async(dst, src, nbytes, stream):
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")  # the runtime torch already loaded
        _hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    rc = _hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), nbytes, 3, C.c_void_p(stream))  # 3 = device to device
    assert rc == 0, rc


class Mailbox:
    """Single-process stand-in for a MATCHED transport (what ncclSend / ncclRecv or batch_isend_irecv are): the `world`
    handles run their shard calls on `world` host threads (ctypes drops the GIL around the library call; the callback
    takes it back), and inside the callbacks rank r's send of call i meets rank r+1's receive of call i -- sends park
    the tail in slot r (a copy on the side stream the library handed over, waited for), everybody meets at a barrier,
    receives copy their predecessor's slot into the landing zone, and a second barrier keeps call i+1's sends out of the
    slots until everyone has read."""

    def __init__(self, world, nbytes):
        import threading
        import torch
        self.world = world
        self.slots = [torch.zeros(nbytes, dtype=torch.uint8, device="cuda") for _ in range(world)]
        self.calls = []
        self.barrier = threading.Barrier(world)

    def exchange_for(self, rank):
        def exchange(d_send, d_recv, nbytes, send_to, recv_from, stream):
            import torch
            self.calls.append((rank, bool(d_send), bool(d_recv), nbytes, send_to, recv_from))
            if send_to >= 0:
                assert d_send
                hip_memcpy_async(self.slots[rank].data_ptr(), d_send, nbytes, stream)
                torch.cuda.synchronize()
            self.barrier.wait(timeout=60)
            if recv_from >= 0:
                assert d_recv
                hip_memcpy_async(d_recv, self.slots[recv_from].data_ptr(), nbytes, stream)
                torch.cuda.synchronize()
            self.barrier.wait(timeout=60)
            return 0
        return exchange

    def run(self, fns):
        """fns[r](): rank r's shard call; all of them at once, like `world` processes."""
        import threading
        out, err = [None] * len(fns), []

        def go(r):
            try:
                out[r] = fns[r]()
            except Exception as e:  # noqa: BLE001
                err.append((r, repr(e)))
                self.barrier.abort()

        ts = [threading.Thread(target=go, args=(r,)) for r in range(len(fns))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not err, err
        return out
