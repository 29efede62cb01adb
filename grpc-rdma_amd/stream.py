"""Device-resident streaming job (grdma_stream_job_*): pushes a whole slice
list through a connected loop-back link with no host round trips."""
import ctypes as C

from ._abi import ReadSlice, Slice, StreamResult
from ._lib import GrdmaError, check, load

u64 = C.c_uint64


RUN_EAGER, RUN_GRAPH, RUN_INSTRUMENTED, RUN_INSTRUMENTED_SCHEDULE = 0, 1, 2, 4
# classes 5 and 6 exist in RUN_INSTRUMENTED_SCHEDULE only: the launches two stages of neighbouring rounds share
CLASS_NAMES = ["tx_plan", "gather", "wire", "rx_plan", "rx_apply", "plan_pair", "scatter_gather"]


class StreamJob:
    def __init__(self, tx, rx, slices, rx_dst_ptr, rx_dst_cap, slices_cap, max_rounds):
        """slices: list of (device ptr, len)."""
        self.lib = load()
        arr = (Slice * len(slices))()
        for i, (p, n) in enumerate(slices):
            arr[i].ptr, arr[i].len = p, n
        self.slices_cap = slices_cap
        self._ends = [(tx, rx)]  # (kept alive: the job's kernels work on the pairs' rings)
        self.h = self.lib.grdma_stream_job_create(tx.h, rx.h, arr, len(slices), rx_dst_ptr,
                                                  rx_dst_cap, slices_cap, max_rounds)
        if not self.h:
            raise GrdmaError(self.lib.grdma_last_error().decode())

    def set_rounds(self, n):
        check(self.lib.grdma_stream_job_set_rounds(self.h, n))

    def set_sends(self, sends):
        """`sends` consecutive Sends per round in one plan (grdma_stream_job_set_sends: rdma_flush's loop while the ring
        has room), paired schedule of a pipelined job."""
        check(self.lib.grdma_stream_job_set_sends(self.h, sends))

    def set_promised_credit(self, on=True):
        """Paired schedule, staged wire: the Send of round t + 1 priced with the credit the drain of round t will post
        (grdma_stream_job_set_promised_credit)."""
        check(self.lib.grdma_stream_job_set_promised_credit(self.h, 1 if on else 0))

    def set_fused_wire(self, on=True):
        """Few links, small rings: the wire of a round inside the planner pair's launch (grdma_stream_job_set_fused_wire)."""
        check(self.lib.grdma_stream_job_set_fused_wire(self.h, 1 if on else 0))

    def wire_groups(self):
        """Wire workgroups per link in the planner pair's launch; 0 = the wire is a launch of its own."""
        return int(self.lib.grdma_stream_job_wire_groups(self.h))

    def set_rebuild_index(self, on=True):
        """The slice tables are rewritten between steps: the index the Sends are priced from is rebuilt in every step
        (grdma_stream_job_set_rebuild_index)."""
        check(self.lib.grdma_stream_job_set_rebuild_index(self.h, 1 if on else 0))

    def set_pipeline(self, on):
        check(self.lib.grdma_stream_job_set_pipeline(self.h, 1 if on else 0))

    def run(self, mode=RUN_GRAPH):
        r = StreamResult()
        check(self.lib.grdma_stream_job_run(self.h, mode, C.byref(r)))
        return r

    def launch(self, streams=False):
        if streams:
            check(self.lib.grdma_stream_job_launch_streams(self.h))
        else:
            check(self.lib.grdma_stream_job_launch(self.h))

    def sync(self):
        check(self.lib.grdma_stream_job_sync(self.h))

    def delivered_slices(self, link=0):
        arr = (ReadSlice * self.slices_cap)()
        n = check(self.lib.grdma_stream_job_slices_of(self.h, link, arr, self.slices_cap))
        return [(int(arr[i].off), int(arr[i].len)) for i in range(n)]

    def close(self):
        if self.h:
            self.lib.grdma_stream_job_destroy(self.h)
            self.h = None


class MultiStreamJob(StreamJob):
    """n links advancing in lock step, one op per link in every launch."""

    def __init__(self, links, max_rounds):
        """links: list of (tx Pair, rx Pair, slices [(ptr,len)...], dst ptr, dst cap, slices cap)."""
        self.lib = load()
        n = len(links)
        self._ends = [(l[0], l[1]) for l in links]  # (kept alive: the job's kernels work on the pairs' rings)
        txs = (C.c_void_p * n)(*[l[0].h for l in links])
        rxs = (C.c_void_p * n)(*[l[1].h for l in links])
        total = sum(len(l[2]) for l in links)
        arr = (Slice * total)()
        k = 0
        for l in links:
            for p, ln in l[2]:
                arr[k].ptr, arr[k].len = p, ln
                k += 1
        counts = (u64 * n)(*[len(l[2]) for l in links])
        dsts = (C.c_void_p * n)(*[l[3] for l in links])
        dcaps = (u64 * n)(*[l[4] for l in links])
        scaps = (u64 * n)(*[l[5] for l in links])
        self.slices_cap = max(l[5] for l in links)
        self.h = self.lib.grdma_stream_job_create_multi(n, txs, rxs, arr, counts, dsts, dcaps, scaps,
                                                        max_rounds)
        if not self.h:
            raise GrdmaError(self.lib.grdma_last_error().decode())
