/* grdma_amd.h -- C ABI of the MI355X-native RDMA_BP/BPEV endpoint data plane.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch
 * types.  Each entry point names the reference interface it replaces (paths
 * relative to the pwrliang/grpc-rdma tree).  INTEGRATION.md shows the C++
 * adapter that fills the real grpc_endpoint_vtable from these calls.
 *
 * Memory model: rings, staging buffers, credit words and the per-connection
 * protocol state live in device HBM.  `grdma_slice.ptr` may point to device
 * memory or to host memory that is device-accessible (hipHostMalloc /
 * hipHostRegister); plain pageable host memory is accepted when the call is
 * flagged GRDMA_MEM_HOST (the library then stages it through a pinned bounce
 * buffer).  All functions return <0 (a negated grdma_error) on failure and
 * never fall back to a CPU implementation: without a usable HIP device
 * grdma_init() fails and every other call reports GRDMA_ERR_NO_DEVICE.
 *
 * Threading (the contract of PairPollable, pair.h:64-81): different pairs may be driven from
 * different threads at the same time; on ONE pair at most one thread sends / writes and at most
 * one thread receives / reads at any moment (never two readers or two writers).  The read-only
 * queries (has_message, has_pending_writes, get_status, readable/writable size, poll_pairs) may
 * run beside them from any thread.  The latency engine's mailbox is serialised inside the
 * library.  grdma_last_error() is per thread.
 */
#ifndef GRDMA_AMD_H
#define GRDMA_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GRDMA_ABI_VERSION 2

enum grdma_error {
  GRDMA_OK = 0,
  GRDMA_ERR_NO_DEVICE = 1,   /* no HIP device / HIP runtime failure at init          */
  GRDMA_ERR_INVALID = 2,     /* bad argument (ring size not a power of two, ...)     */
  GRDMA_ERR_HIP = 3,         /* a HIP call failed; see grdma_last_error()            */
  GRDMA_ERR_NOT_CONNECTED = 4,
  GRDMA_ERR_CAPACITY = 5,    /* slice list / arena larger than the configured caps   */
  GRDMA_ERR_CONFIG = 6,      /* GRPC_PLATFORM_TYPE / GRPC_RDMA_* value rejected      */
  GRDMA_ERR_AGAIN = 7        /* an asynchronous operation has not completed yet       */
};

/* ---- platform selection: src/core/lib/iomgr/iomgr_internal.cc:37-62 --------- */
enum grdma_platform {          /* iomgr_internal.h:45 platform_t */
  GRDMA_IOMGR_TCP = 0,
  GRDMA_IOMGR_RDMA_BP = 1,
  GRDMA_IOMGR_RDMA_BPEV = 2,
  GRDMA_IOMGR_RDMA_EVENT = 3
};
/* Parses a GRPC_PLATFORM_TYPE value: NULL/unset -> TCP, exact strings "TCP",
 * "RDMA_BP", "RDMA_BPEV", "RDMA_EVENT"; anything else -> -GRDMA_ERR_CONFIG
 * (the reference calls exit(1) there, iomgr_internal.cc:57-58). */
int grdma_parse_platform(const char* value);
/* grpc_determine_iomgr_platform(): reads the environment once. */
int grdma_determine_platform(void);

/* ---- Config: src/core/lib/ibverbs/config.cc:45-115 --------------------------- */
typedef struct grdma_config {
  char device_name[64];              /* GRPC_RDMA_DEVICE_NAME   ("" = first)      */
  int32_t port_num;                  /* GRPC_RDMA_PORT_NUM      (1)               */
  int32_t gid_index;                 /* GRPC_RDMA_GID_INDEX     (0)               */
  int32_t poller_thread_num;         /* GRPC_RDMA_POLLER_THREAD_NUM (1)           */
  int32_t busy_polling_timeout_us;   /* GRPC_RDMA_BUSY_POLLING_TIMEOUT_US (500)   */
  int32_t poller_sleep_timeout_ms;   /* GRPC_RDMA_POLLER_SLEEP_TIMEOUT_MS (1000)  */
  uint32_t ring_buffer_size_kb;      /* GRPC_RDMA_RING_BUFFER_SIZE_KB (4096)      */
  uint32_t zerocopy_buffer_size_kb;  /* reads the SAME variable (config.cc:100-106), 32768 */
  uint32_t zerocopy_threshold_kb;    /* GRPC_RDMA_ZEROCOPY_THRESHOLD_KB (UINT32_MAX) */
  int32_t max_sge;                   /* GRPC_RDMA_MAX_SGE: this build's stand-in for
                                        the HCA attribute max_sge (pair.cc:53-60); 30 */
  int32_t hip_device;                /* GRPC_RDMA_HIP_DEVICE (LOCAL_RANK or 0)    */
  int32_t hip_wire_direct;           /* GRPC_RDMA_HIP_WIRE: "direct" (1, default: records are encoded straight into
                                        the peer ring -- every wire of this build is device memory the sender can
                                        address) or "staged" (0: through the ring/2 staging buffer and <= 2 wire
                                        writes, what a NIC posts)                                          */
  uint32_t hip_register_min;         /* GRPC_RDMA_HIP_REGISTER_MIN: host slices of at least this many bytes are read
                                        where they lie (pages registered once), 0 = always copied (default) */
  uint32_t hip_pair_pool_mb;         /* GRPC_RDMA_HIP_PAIR_POOL_MB: how much memory of closed connections the PairPool
                                        keeps for the next ones (default 4096; 0 = none)                    */
} grdma_config;
int grdma_config_from_env(grdma_config* out);

/* ---- library / device ------------------------------------------------------------ */
int grdma_init(int hip_device);      /* Device::Get(), device.cc:45-101           */
int grdma_device_count(void);
const char* grdma_last_error(void);
int grdma_abi_version(void);

/* ---- PairPollable: src/core/lib/ibverbs/pair.h:106-152 ---------------------- */
typedef struct grdma_pair grdma_pair;

typedef struct grdma_slice {         /* GRPC_SLICE_START_PTR / GRPC_SLICE_LENGTH  */
  const void* ptr;
  uint64_t len;
} grdma_slice;

enum grdma_flags {
  GRDMA_MEM_DEVICE = 0,   /* slice pointers are device-accessible                  */
  GRDMA_MEM_HOST = 1,     /* pageable host memory: stage through the bounce buffer */
  GRDMA_WIRE_STAGED = 0,  /* records are built in the staging buffer, then written
                             to the peer ring by <=2 wire writes (what a NIC needs) */
  GRDMA_WIRE_DIRECT = 2,  /* loop-back / xGMI peer: encode straight into the ring  */
  GRDMA_WIRE_ORDERED = 8, /* what writes into THIS pair's ring places the bytes of a write in address order, the
                             footer last -- an RDMA NIC (the reference's wire): header + footer say "complete",
                             as ring_buffer.cc:67-97 assumes.  Without the flag the writer is taken to be a HIP
                             wire (copy kernel, IPC / xGMI peer): a PARALLEL copy, whose sender reports how far
                             its completed writes reach (csrc/grdma_dev.h: grdma_wire_report) and whose receiver
                             never walks past that report */
  GRDMA_RING_FINE_GRAINED = 4  /* allocate the ring (and the connection block holding the 16-byte
                             status report) as fine-grained device memory
                             (hipExtMallocWithFlags, hipDeviceMallocFinegrained): stores are
                             write-through and visible to a peer device / process / NIC once
                             acknowledged, with no cache maintenance at kernel boundaries --
                             what a ring registered for remote writes needs */
};

/* PairPollable() + Init(): allocates the HBM ring (ring_size bytes, power of
 * two > 24, ring_buffer.cc:22-24), the ring/2 staging buffer (pair.cc:104), the
 * status words and a receive arena.  pair.cc:21-76, 85-141. */
grdma_pair* grdma_pair_create(uint64_t ring_size, int max_sge, int flags);
/* Connect(): the loop-back wire replaces the 48-byte address exchange + QP
 * bring-up (rdma_bp_posix.cc:767-771, pair.cc:143-168).  Both ends must use the
 * same ring size (asserted at pair.cc:149). */
int grdma_pair_connect(grdma_pair* a, grdma_pair* b);
/* Bootstrap between processes / GPUs.  The reference swaps a 48-byte Address over the TCP fd
 * (exchange_data, rdma_bp_posix.cc:640-692,767-771; layout address.h:24-31), checks tag and ring
 * size in Connect() (pair.cc:143-149), brings the QP up and swaps the memory regions of ring and
 * status buffer (syncMemoryRegion).  Here the memory region of an HBM ring is a HIP IPC handle
 * (the same allocation exports as a dma-buf for a NIC); both travel in one blob whose first 48
 * bytes are the reference's Address.  export -> send/recv over any byte channel -> connect_remote,
 * or grdma_pair_bootstrap_fd() which does all three over a connected socket like
 * grpc_rdma_bp_create does (rdma_bp_posix.cc:763-784). */
typedef struct grdma_address {          /* address.h:24-31 (48 bytes, natural alignment)          */
  uint32_t lid, qpn, psn, pad0;
  uint8_t gid[16];                      /* union ibv_gid; here: PCI bus id of the HIP device      */
  uint32_t tag, pad1;                   /* 0xa0: peers must agree (pair.cc:72,146)                */
  uint64_t ring_buffer_size;            /* peers must agree (pair.cc:107,147-149)                 */
} grdma_address;
typedef struct grdma_bootstrap_blob {
  grdma_address addr;
  uint32_t magic, version;              /* "GRDM", GRDMA_ABI_VERSION                              */
  int32_t hip_device;
  uint32_t wire_off;                    /* offset of the arrival report (grdma_wire_report) in the conn block */
  uint64_t pid;
  uint64_t status_off;                  /* offset of the 16-byte status_report in the conn block  */
  uint8_t ring_handle[64];              /* hipIpcMemHandle_t of the ring                          */
  uint8_t conn_handle[64];              /* hipIpcMemHandle_t of the connection block              */
} grdma_bootstrap_blob;
int grdma_pair_export_address(grdma_pair* p, grdma_bootstrap_blob* out);
int grdma_pair_connect_remote(grdma_pair* p, const grdma_bootstrap_blob* peer);
int grdma_pair_bootstrap_fd(grdma_pair* p, int fd);
int grdma_pair_disconnect(grdma_pair* p);          /* Disconnect(), pair.cc:325-347 */
void grdma_pair_destroy(grdma_pair* p);

/* ---- PairPool (src/core/lib/ibverbs/pair.h:273-333: Take(id) / Get(id) / Putback over pre-built pairs) --------
 * Here the pool keeps the MEMORY of released pairs (ring, staging, plans, arena, pinned blocks) by size and
 * hands it to the next grdma_pair_create / _take of the same shape, and maps connection ids to pairs. */
int grdma_pair_pool_reserve(uint32_t pairs, uint64_t ring_size, int max_sge, int flags, uint64_t cap_bytes);
grdma_pair* grdma_pair_pool_take(const char* id, uint64_t ring_size, int max_sge, int flags);  /* PairPool::Take  */
grdma_pair* grdma_pair_pool_get(const char* id);                                              /* PairPool::Get   */
void grdma_pair_pool_putback(grdma_pair* p);                                                  /* PairPool::Putback */
int grdma_pair_pool_stats(uint64_t out[5]);  /* blocks held, bytes held, pool hits, runtime allocations, ids registered */
void grdma_pair_pool_trim(void);
/* PairStatus, pair.h:44-51: the values grdma_pair_get_status returns */
#ifndef GRDMA_PAIR_STATUS_DEFINED
#define GRDMA_PAIR_STATUS_DEFINED
enum grdma_pair_status {
  GRDMA_PAIR_UNINITIALIZED = 0,
  GRDMA_PAIR_INITIALIZED = 1,
  GRDMA_PAIR_CONNECTED = 2,
  GRDMA_PAIR_HALF_CLOSED = 3,
  GRDMA_PAIR_DISCONNECTED = 4,
  GRDMA_PAIR_ERROR = 5
};
#endif
int grdma_pair_get_status(grdma_pair* p);          /* get_status(), pair.cc:349-375 */

/* Send(slices, count, byte_idx), pair.cc:645-734.  Returns payload bytes
 * accepted (a prefix of the slice list) or <0. */
int64_t grdma_pair_send(grdma_pair* p, const grdma_slice* slices, uint64_t count,
                        uint64_t byte_idx, int flags);
/* Recv(buf, capacity), pair.cc:264-286: one RingBufferPollable::Read.  dst is
 * device-accessible memory (or host memory with GRDMA_MEM_HOST). */
int64_t grdma_pair_recv(grdma_pair* p, void* dst, uint64_t capacity, int flags);
int grdma_pair_has_message(grdma_pair* p);         /* HasMessage(), ring_buffer.cc:56-65   */
int grdma_pair_has_pending_writes(grdma_pair* p);  /* HasPendingWrites(), pair.cc:303      */
int64_t grdma_pair_readable_size(grdma_pair* p);   /* GetReadableSize(), ring_buffer.cc:67 */
int64_t grdma_pair_writable_size(grdma_pair* p);   /* GetWritableSize(), pair.cc:294-301   */

/* Zero-copy send buffer (pair.h:96,127,140; pair.cc:103-120, 305-323, 793-941).
 * grdma_pair_enable_zerocopy   initSendBuffer(kZeroCopyBuffer): `bytes` owned by the pair (0 =
 *                              GRPC_RDMA_ZEROCOPY_BUFFER_SIZE_KB as the reference's Config reads it);
 *                              allocate_send_buffer enables it on first use.  HOST-WRITABLE and device-readable:
 *                              the reference's caller serialises into it with the CPU (GenericSerialize ->
 *                              SerializeWithCachedSizesToArray, include/grpcpp/impl/codegen/proto_utils.h:68-95, through
 *                              CoreCodegen::grpc_call_allocate_send_buffer, src/cpp/common/core_codegen.cc:122-146).
 *                              _ex names the memory: GRDMA_ZC_MEM_HOST (pinned mapped host memory, the default: the
 *                              gather pulls the payload over PCIe into the peer ring), GRDMA_ZC_MEM_BAR (fine-grained
 *                              device memory the CPU writes through the PCIe BAR), GRDMA_ZC_MEM_DEVICE (device memory
 *                              for serialisers that run on the device; not host-writable).  Environment:
 *                              GRPC_RDMA_HIP_ZEROCOPY_MEM = host | bar | device.
 * grdma_pair_allocate_send_buffer  AllocateSendBuffer(size): a pointer into that buffer, or NULL
 *                              when size == 0, the buffer is not empty (the reference serves one
 *                              allocation at a time: tail != 0 -> nullptr) or the size does not fit.
 *                              The caller serialises its message there (plain CPU stores for HOST / BAR).
 * grdma_pair_send_zerocopy     SendZerocopy(slices, count, byte_idx): a slice that lies inside the
 *                              zero-copy buffer becomes a record whose payload is read where it lies
 *                              (limited by the receiver's credit only; the reference stages 16 +
 *                              padding tag bytes and uses 4 of its max_sge entries for it), any other
 *                              slice is priced as Send prices it.  GRDMA_MEM_DEVICE: every slice is device-
 *                              accessible; GRDMA_MEM_HOST: the slices are the host's (what grpc_endpoint_write hands
 *                              over) -- ranges of the zero-copy buffer are still read in place, the others are
 *                              copied through the pinned bounce buffer as grdma_pair_send does.
 *                              Returns the payload bytes accepted; partial_write, remote_tail and the
 *                              <= 2 work requests (grdma_pair_last_wrs) as the reference leaves them.
 *                              On this wire every record of the call goes straight from its source into
 *                              the peer ring (one gather launch); nothing is written to the staging buffer.
 * grdma_pair_zerocopy_state    out = {zerocopy_buffer_tail_, zerocopy_bytes_, copy_bytes_, scatter-gather
 *                              entries the reference's list would hold after the last call}. */
enum grdma_zc_mem { GRDMA_ZC_MEM_HOST = 0, GRDMA_ZC_MEM_BAR = 1, GRDMA_ZC_MEM_DEVICE = 2 };
int grdma_pair_enable_zerocopy(grdma_pair* p, uint64_t bytes);
int grdma_pair_enable_zerocopy_ex(grdma_pair* p, uint64_t bytes, int mem);
int grdma_pair_zerocopy_mem(grdma_pair* p);   /* the kind of the buffer in use, or -1 */
void* grdma_pair_allocate_send_buffer(grdma_pair* p, uint64_t size);
int64_t grdma_pair_send_zerocopy(grdma_pair* p, const grdma_slice* slices, uint64_t count,
                                 uint64_t byte_idx, int flags);
int grdma_pair_zerocopy_state(grdma_pair* p, uint64_t out[4]);

/* Observability used by the parity tests (debug monitor of pair.h:235-270). */
typedef struct grdma_pair_state {
  uint64_t head, moving_head, remain;              /* ring_buffer.h:203-205 */
  uint64_t remote_tail, remote_head;               /* pair.h:170, 229-233   */
  uint64_t internal_read_size, credit_msgs, partial_write;
  uint64_t total_read, total_written, leftover_cap;
} grdma_pair_state;
int grdma_pair_state_get(grdma_pair* p, grdma_pair_state* out);
/* Copies `len` bytes of the pair's HBM ring / staging buffer to host memory. */
int grdma_pair_peek_ring(grdma_pair* p, uint64_t off, void* host_dst, uint64_t len);
int grdma_pair_peek_staging(grdma_pair* p, uint64_t off, void* host_dst, uint64_t len);
/* Last Send's work requests {remote ring offset, length}; returns the count
 * (GetWriteRequests, ring_buffer.cc:261-330). */
int grdma_pair_last_wrs(grdma_pair* p, uint64_t out[2][2]);
void* grdma_pair_ring_device_ptr(grdma_pair* p);

/* ---- background poller (RDMA_BPEV): src/core/lib/ibverbs/poller.h:16-71, poller.cc:12-106 ----
 * n_threads host threads (GRPC_RDMA_POLLER_THREAD_NUM, must be > 0) share one round-robin cursor over the
 * slot table, as the reference's do (poller.cc:66-69).  What a thread looks at is the pair's host-visible
 * state line -- no device work for a pair whose peer lives in this process.  A pair's wakeup fd (an
 * eventfd; the reference's grpc_wakeup_fd, pair.h:150,187) becomes readable when the pair is connected
 * and readable or writable (a message, a completed drain or Send, credit for a parked write), or when it
 * is half-closed / in error (poller.cc:80-98); it is not signalled again until the consumer has read it
 * (poller.cc:76-78).  The event engine adds the fd to its epoll set exactly as
 * ev_epollex_rdma_bpev_linux.cc does.  sleep_timeout_ms mirrors GRPC_RDMA_POLLER_SLEEP_TIMEOUT_MS. */
typedef struct grdma_poller grdma_poller;
grdma_poller* grdma_poller_create(int n_threads, int sleep_timeout_ms);
void grdma_poller_destroy(grdma_poller* pl);                 /* Poller::Shutdown          */
int grdma_poller_add(grdma_poller* pl, grdma_pair* p);       /* AddPollable; returns the fd */
int grdma_poller_remove(grdma_poller* pl, grdma_pair* p);    /* RemovePollable; afterwards the
                                                              * poller no longer touches p   */
int grdma_poller_stats(grdma_poller* pl, uint64_t* passes, uint64_t* wakeups);
int grdma_poller_threads(grdma_poller* pl);                  /* threads running (GRPC_RDMA_POLLER_THREAD_NUM) */
int grdma_pair_get_wakeup_fd(grdma_pair* p);                 /* PairPollable::get_wakeup_fd */
int grdma_pair_consume_wakeup(grdma_pair* p);                /* grpc_wakeup_fd_consume_wakeup: 1 if one was pending */

/* ---- endpoint read/write on the pair: rdma_bp_posix.cc ----------------------- */
typedef struct grdma_read_slice { uint64_t off, len; } grdma_read_slice;

/* rdma_write()/rdma_flush() (rdma_bp_posix.cc:470-586): sends as much of the
 * slice list as credit allows, continuing from the internal cursor
 * (outgoing_byte_idx).  *done = 1 when the whole buffer went out; otherwise the
 * caller retries when the pair becomes writable (notify_on_write). */
int64_t grdma_endpoint_write_begin(grdma_pair* p, const grdma_slice* slices, uint64_t count,
                                   int flags);
int64_t grdma_endpoint_write_step(grdma_pair* p, int* done);
/* Forget the outstanding write (the error exits of rdma_flush, :505-517, unref the slice
 * buffer; afterwards a new grdma_endpoint_write_begin is accepted). */
int grdma_endpoint_write_abort(grdma_pair* p);

/* rdma_read()/rdma_continue_read()/rdma_do_read() (rdma_bp_posix.cc:180-376):
 * performs up to max_reads endpoint_read completions in ONE device pass; each
 * completion is one slice in the pair's receive arena.  Returns the number of
 * completions; slices[i] = {arena offset, length}.  *would_block = 1 when the
 * last attempt found no complete record (the endpoint re-arms notify_on_read). */
int64_t grdma_endpoint_read(grdma_pair* p, uint64_t max_reads, grdma_read_slice* slices,
                            uint64_t slices_cap, int* would_block);
/* ---- asynchronous endpoint operations ----------------------------------------------------------
 * What the grpc_endpoint_vtable adapter runs on (include/grdma_endpoint_impl.hpp).  grpc_endpoint_write and
 * grpc_endpoint_read return once the device work is enqueued -- a launch chain on the pair's send / receive stream,
 * or one command to the resident latency engine when the pair is in latency mode --; the completion shows up in
 * pinned host memory and the event engine's poll loop finds it with plain loads (grdma_endpoint_readable /
 * _writable are what HasMessage() / HasPendingWrites() mean to ev_epollex_rdma_bp{,ev}_linux.cc for such an
 * endpoint).  Delivered slices lie in receive windows of pinned host memory that the scatter kernel writes over
 * PCIe: the transport gets slices that POINT into the window (no copy on the host), each holding a reference.
 * One Send and one drain in flight per pair; the blocking calls above must not be mixed in while one is.
 *
 * grdma_endpoint_set_async(p, windows, window_bytes)  windows >= 2 (0 = 3); window_bytes 0 = sized from the ring.
 * grdma_endpoint_write_submit(p)    one rdma_flush step (a Send from the cursor of the begun write), not waited for.
 * grdma_endpoint_write_test(p, &done, &sent)   1: the step completed (as grdma_endpoint_write_step reports it),
 *                                   0: still in flight, < 0: error.
 * grdma_endpoint_read_submit(p, max_reads)     0: a drain of up to max_reads endpoint reads is on its way,
 *                                   1: every window still holds slices the transport has not released.
 * grdma_endpoint_read_test(p, slices, cap, &would_block, &window)   >= 0: completions, slices[i].off relative to
 *                                   grdma_window_base(window); the caller owns one reference of the window
 *                                   (grdma_window_unref when the last slice is gone); -GRDMA_ERR_AGAIN: in flight.
 * grdma_pair_arm_read(p, n) on an asynchronous pair in latency mode: a standing read order with a watcher workgroup of
 *                                   the resident engine, carried out when bytes land in the pair's ring (whoever wrote
 *                                   them); to the endpoint it is a drain in flight that completes by itself. */
typedef struct grdma_window grdma_window;
int grdma_endpoint_set_async(grdma_pair* p, int windows, uint64_t window_bytes);
int grdma_endpoint_write_submit(grdma_pair* p);
int grdma_endpoint_write_test(grdma_pair* p, int* done, int64_t* sent);
/* A write submitted BEHIND the burst in flight (asynchronous endpoint, direct wire, a write of more slices than
 * max_sge and at most 16 x max_sge): its chain goes into the send stream now and runs only if the write in front
 * turns out to have gone out whole (gated on the device); slices must be device-visible and stay valid.
 * _queue: 0 = queued, 1 = not possible now.  _adopt, after grdma_endpoint_write_test reported the write in front
 * complete: 1 = the queued write is the outstanding one now, its burst in flight; 0 = it has to be submitted the
 * ordinary way (never queued, or skipped because the write in front came up short). */
int grdma_endpoint_write_queue(grdma_pair* p, const grdma_slice* slices, uint64_t count);
int grdma_endpoint_write_adopt(grdma_pair* p);
int grdma_endpoint_write_queue_stats(grdma_pair* p, uint64_t out[3]);  /* queued, promoted, skipped */
int grdma_endpoint_write_queue_limits(grdma_pair* p, uint64_t out[2]); /* slices, bytes one queued write may hold */
int grdma_endpoint_write_quiesce(grdma_pair* p);  /* nothing of this pair's is left in its send stream when it returns */
int grdma_endpoint_read_submit(grdma_pair* p, uint64_t max_reads);
int64_t grdma_endpoint_read_test(grdma_pair* p, grdma_read_slice* slices, uint64_t slices_cap, int* would_block,
                                 grdma_window** window);
int grdma_endpoint_read_idle(grdma_pair* p);      /* an endpoint read found nothing and submitted no drain: the 256-byte
                                                     slice it allocated stays for the next edge (rdma_bp_posix.cc:283-287) */
int grdma_endpoint_readable(grdma_pair* p);
int grdma_endpoint_writable(grdma_pair* p);
int grdma_endpoint_busy(grdma_pair* p);           /* 1: a Send or a drain of this pair is on the device and has not
                                                     completed yet (an event loop running a connection to quiescence) */
int grdma_endpoint_drain_state(grdma_pair* p);    /* 0: no drain in flight, 1: in flight, 2: completed, not collected
                                                     (a drain may have been posted by the in-process peer's sender
                                                     on behalf of an armed read) */
int grdma_endpoint_free_windows(grdma_pair* p);   /* receive windows no slice of the transport points into */
const void* grdma_window_base(const grdma_window* w);
void grdma_window_ref(grdma_window* w);
void grdma_window_unref(grdma_window* w);
/* GRDMA_MEM_HOST slices of at least this many bytes are read where they lie -- the library registers their pages
 * with the device once (hipHostRegister) and remembers the registration -- instead of being copied into the
 * pinned bounce buffer.  0 (default) = always copy.  The caller guarantees that a registered range stays mapped
 * (memory handed back to the OS must be announced with grdma_forget_host_range first).  Env: GRPC_RDMA_HIP_REGISTER_MIN. */
int grdma_set_host_register_min(uint64_t bytes);
int grdma_forget_host_range(const void* ptr, uint64_t len);

/* Export the ring as a dma-buf file descriptor (hipMemGetHandleForAddressRange,
 * hipMemRangeHandleTypeDmaBufFd): what ibv_reg_dmabuf_mr() takes to register the HBM ring with an
 * RDMA NIC -- the place of ibv_reg_mr() in the reference (rdma_utils.h:108-160, pair.cc:107-119).
 * Returns the fd (owned by the caller: close() it) or < 0. */
int grdma_pair_export_ring_dmabuf(grdma_pair* p);
/* ---- NIC wire (ibverbs): what PairPollable's verbs calls are in the reference --------------------------------
 * grdma_pair_verbs_open     Init(): device, protection domain, completion queue, queue pair; ring and status block
 *                           registered remote-writable -- the ring through its dma-buf where the verbs library has
 *                           ibv_reg_dmabuf_mr -- staging buffer and status_send as local regions (pair.cc:107-119,
 *                           rdma_utils.h:108-160).  The pair must have been created with GRDMA_WIRE_ORDERED (a NIC places
 *                           the bytes of a write in order, footer last) and without GRDMA_WIRE_DIRECT.
 * grdma_pair_verbs_address  what the reference's Address carries for this end (pair.h:53-98): queue pair number, lid,
 *                           gid, ring and status addresses with their rkeys.
 * grdma_pair_verbs_connect  Connect(peer): RESET -> INIT -> RTR -> RTS (pair.cc:143-262); the pair is kConnected and
 *                           from then on a Send's <= 2 chained IBV_WR_RDMA_WRITEs (pair.cc:709-734: what the send planner
 *                           left in grdma_pair_last_wrs) and a drain's 16-byte status write (updateStatus, :624-641) are
 *                           posted through the queue pair and reaped (csrc/grdma_wire_verbs.cc).
 * Libraries built without <infiniband/verbs.h> (grdma_verbs_supported() == 0) report an error from _open. */
typedef struct grdma_verbs_address {
  uint32_t qpn, psn;
  uint16_t lid;
  uint16_t pad0;
  uint32_t ring_rkey;
  uint8_t gid[16];
  uint64_t ring_addr, ring_size;
  uint64_t status_addr;
  uint32_t status_rkey, status_size;
} grdma_verbs_address;
int grdma_verbs_supported(void);
int grdma_pair_verbs_open(grdma_pair* p, const char* device, int port, int gid_index);
int grdma_pair_verbs_address(grdma_pair* p, grdma_verbs_address* out);
int grdma_pair_verbs_connect(grdma_pair* p, const grdma_verbs_address* peer);
int grdma_pair_verbs_counts(grdma_pair* p, uint64_t out[3]);  /* data writes posted, status writes posted, completions reaped */
void* grdma_pair_arena_device_ptr(grdma_pair* p);
uint64_t grdma_pair_arena_size(grdma_pair* p);
int grdma_pair_arena_copy_out(grdma_pair* p, uint64_t off, void* host_dst, uint64_t len);

/* ---- latency path ------------------------------------------------------------------------
 * Latency mode: every blocking call becomes ONE fused kernel launch (the planning
 * workgroup also moves the bytes), the host waits on a sequence word in pinned
 * memory instead of a stream synchronize, and delivered slices are written
 * straight into a pinned host arena. */
int grdma_pair_set_latency_mode(grdma_pair* p, int on);
/* Standing read order: what an outstanding grpc_endpoint_read is to the reference's busy-polling thread
 * (rdma_bp_posix.cc:345-372 arms it, the poller completes it when a record lands, ring_buffer.cc:56-97).
 * "grdma_endpoint_read(max_reads) into the next free window, whenever there is something": the order sits in one
 * of the resident engine's 64 watch slots; a watcher workgroup polls the arrival report of THIS pair's ring and
 * drains when it moves -- whoever wrote the bytes (the in-process peer, another process over IPC, a NIC) --, and the
 * next grdma_endpoint_read (max_reads >= the armed value) finds the completion in pinned memory without a command
 * of its own.  Same bytes, order and state as a read issued at that moment.  Latency mode only; not on a NIC-wire
 * pair.  max_reads = 0 takes the order back.  One reading thread per pair. */
int grdma_pair_arm_read(grdma_pair* p, uint64_t max_reads);
int64_t grdma_pair_watch_hits(const grdma_pair* p);   /* completions a watcher workgroup produced and a read took */
int grdma_engine_watchers(void);                      /* watcher workgroups per engine incarnation (GRDMA_ENGINE_WATCHERS) */
int grdma_pair_armed_ready(const grdma_pair* p);      /* 1: a completion is waiting (host memory only: no device work) */
/* Persistent latency engine: one resident workgroup takes the fused Send / drain
 * commands of latency-mode pairs from a mailbox in pinned host memory (a PCIe
 * doorbell read instead of a kernel launch per call).  It retires by itself after
 * ~1 s without commands; stop it before any device-wide synchronize. */
int grdma_engine_start(void);
int grdma_engine_stop(void);
/* Unary ping-pong (the reference's micro-bench loop, examples/cpp/micro-bench/mb_client.cc):
 * a = client end, b = server end of a connected link.  rtt_ns has `iters` entries. */
int grdma_pingpong(grdma_pair* a, grdma_pair* b, const grdma_slice* req, uint64_t nreq,
                   const grdma_slice* resp, uint64_t nresp, int mem_flags, uint64_t iters,
                   uint64_t warmup, uint64_t* rtt_ns, uint64_t phase_ns[4]);

/* One END of a unary ping-pong whose other end lives in another process (the rings mapped through IPC handles,
 * grdma_pair_bootstrap_fd): is_client = write `out`, then read until in_bytes have arrived; server = the other way
 * round.  With a standing read order (grdma_pair_arm_read) the bytes the OTHER process wrote into this pair's ring are
 * found by a watcher workgroup of this process's engine.  byte_sum = sum of every byte received. */
int grdma_pingpong_end(grdma_pair* p, int is_client, const grdma_slice* out, uint64_t nout, uint64_t in_bytes, int mem_flags,
                       uint64_t iters, uint64_t warmup, uint64_t* rtt_ns, uint64_t* byte_sum);

/* ---- K3 batched message-ready detection ------------------------------------------- */
/* HasMessage()/GetReadableSize() for n pairs in one launch (the busy-poll scan
 * of ev_epollex_rdma_bpev_linux.cc:1105-1149 / poller.cc:84).  readable[i] = bytes,
 * has_message[i] = 0/1. */
int grdma_poll_pairs(grdma_pair* const* pairs, uint32_t n, uint64_t* readable,
                     uint8_t* has_message);

/* ---- device-resident streaming job ------------------------------------------------
 * Pushes a whole slice list (e.g. a batch of framed gRPC messages) through a
 * connected loop-back link without host round trips: each round is one
 * rdma_flush step on `tx` (Send from the device-side cursor), the wire write,
 * and one drain of `rx` (as many endpoint_read completions as are ready),
 * appended to rx_dst.  This is the reference's write loop
 * (rdma_bp_posix.cc:470-557) and read loop (:180-376) with the credit
 * hand-shake of pair.cc:264-301 between them, enqueued back to back. */
typedef struct grdma_stream_job grdma_stream_job;
typedef struct grdma_stream_result {
  uint64_t bytes_sent, bytes_delivered, slices_delivered;
  uint64_t tx_rounds, rx_rounds, tx_records, rx_records;
  uint64_t done;               /* 1: every slice was sent and delivered            */
  double ms_total;             /* HIP-event time of the enqueued rounds            */
  double ms_class[8];          /* instrumented modes: summed kernel time per class */
  uint64_t launches_class[8];  /*   0 tx_plan 1 gather 2 wire 3 rx_plan 4 rx_apply (scatter+zero+credit)
                                *   _INSTRUMENTED_SCHEDULE also: 5 plan_pair (drain plan of round t + send plan of
                                *   round t + 1, one launch) 6 scatter_gather (scatter of round t + gather of t + 1) */
} grdma_stream_result;
enum grdma_stream_mode {
  GRDMA_RUN_EAGER = 0, GRDMA_RUN_GRAPH = 1, GRDMA_RUN_INSTRUMENTED = 2,
  /* (3 was the persistent link engine, k_link: one resident launch per step -- a third of the graph schedule's rate in
   *  rounds 2 - 4, retired in round 5; profiles/r04_bench_engine_*) */
  /* The launches of the default (pipelined, paired) schedule one after the other on one stream with a HIP event
   * between every two: the graph's order is a chain already, so the work and its order are the graph's; the
   * events give the time of every launch by itself.  GRDMA_ERR_INVALID for a job that is not on that schedule. */
  GRDMA_RUN_INSTRUMENTED_SCHEDULE = 4
};

grdma_stream_job* grdma_stream_job_create(grdma_pair* tx, grdma_pair* rx,
                                          const grdma_slice* slices, uint64_t count,
                                          void* rx_dst, uint64_t rx_dst_cap,
                                          uint64_t slices_cap, uint64_t max_rounds);
/* n independent links advancing in lock step: every kernel launch carries one op
 * per link (connections are the data-parallel axis; config 4 =
 * 32 connections per GPU).  slices holds the links' slice lists back to back,
 * counts[i] entries each. */
grdma_stream_job* grdma_stream_job_create_multi(uint32_t n, grdma_pair* const* tx,
                                                grdma_pair* const* rx, const grdma_slice* slices,
                                                const uint64_t* counts, void* const* rx_dsts,
                                                const uint64_t* rx_dst_caps,
                                                const uint64_t* slices_caps, uint64_t max_rounds);
int grdma_stream_job_slices_of(grdma_stream_job* j, uint32_t link, grdma_read_slice* out, uint64_t cap);
void grdma_stream_job_destroy(grdma_stream_job* j);
int grdma_stream_job_run(grdma_stream_job* j, int mode, grdma_stream_result* out);
/* Asynchronous form for timed loops: enqueue one pass (the captured graph) on
 * the link's stream without reading any state back; _sync() waits for it. */
int grdma_stream_job_launch(grdma_stream_job* j);
/* Same work as _launch, issued kernel by kernel on the job's streams (no graph). */
int grdma_stream_job_launch_streams(grdma_stream_job* j);
int grdma_stream_job_sync(grdma_stream_job* j);
int grdma_stream_job_slices(grdma_stream_job* j, grdma_read_slice* out, uint64_t cap);
int grdma_stream_job_set_rounds(grdma_stream_job* j, uint64_t rounds);
/* on != 0: neighbouring rounds share launches, the way two hosts and a NIC work on different rounds at once: the
 * drain plan of round t with the send plan of round t + 1 (k_plan_pair_mw), the scatter of round t with the
 * gather of round t + 1 (k_rx_apply_gather), the wire in between -- three launches per round; two with a direct
 * wire, or with the wire inside the planner pair's launch (grdma_stream_job_set_fused_wire: few links, rings of at
 * most 16 MiB) (DESIGN.md sections 2.5, 2.9).  A drain walks exactly up to the tail its own Send reported; the sender may see a
 * credit one round later than in the sequential schedule.  Same bytes delivered; affects GRDMA_RUN_GRAPH, _EAGER
 * and _INSTRUMENTED_SCHEDULE. */
int grdma_stream_job_set_pipeline(grdma_stream_job* j, int on);
/* `sends` (1..64) consecutive Sends per round in ONE plan -- rdma_flush's loop while the ring has room
 * (rdma_bp_posix.cc:470-524): Send, advance the cursor, Send again -- before the peer drains; paired schedule of a
 * pipelined job only (other schedules keep one Send per round).  Up to two Sends are priced one after the other;
 * more (small max_sge: the reference's default is 30) as one cut of the slice table's index. */
int grdma_stream_job_set_sends(grdma_stream_job* j, uint32_t sends);
/* Paired schedule, staged wire: price the Send of round t + 1 with the credit the drain of round t will post (it waits
 * for that drain's plan inside the launch they share) -- no round of credit lag at a ring every round fills. */
int grdma_stream_job_set_promised_credit(grdma_stream_job* j, int on);
/* Paired schedule, staged wire, a job of few links with rings of at most 16 MiB: the wire of a round rides in the launch
 * of the planner pair (wire workgroups of k_plan_pair_mw; the drain's workgroups wait for them before they look at the
 * ring) instead of a k_copy launch of its own -- two launches per round.  On by default where every workgroup of that
 * launch has a CU at once; this call with on = 0 turns it off.  The getter says how many wire workgroups per link the
 * job's graph carries (0: the wire is a launch of its own). */
int grdma_stream_job_set_fused_wire(grdma_stream_job* j, int on);
uint32_t grdma_stream_job_wire_groups(grdma_stream_job* j);
/* The job's slice tables are rewritten between steps (every grpc_endpoint_write brings a new slice buffer,
 * rdma_bp_posix.cc:559-586): the index its Sends are priced from (k_tx_index: prefix sums over the table) is rebuilt
 * in EVERY step's first round instead of once per job.  bench.py times both. */
int grdma_stream_job_set_rebuild_index(grdma_stream_job* j, int on);

/* ---- diagnostics (profiling aids used by tools/; not needed by an integration) ------------
 * s_memtime stamps / counters the plan kernels leave in their result blocks, the
 * record-size history of a pair, per-command cycle counts of the latency engine. */
int grdma_pair_last_dbg(grdma_pair* p, uint64_t tx_dbg[16], uint64_t rx_dbg[16]);
int grdma_stream_job_debug(grdma_stream_job* j, uint64_t tx_dbg[16], uint64_t rx_dbg[16]);
int grdma_pair_debug_hist(grdma_pair* p, uint32_t* hist_out /* 1024 entries */, uint64_t* count,
                          uint32_t* period);
int grdma_engine_debug(uint64_t out[5]);
uint64_t grdma_express_drains(void);  /* drains served by the single-wave express path so far */
uint64_t grdma_watch_fast_drains(void);      /* diagnostics: drains the watchers' single-wave path took */
int grdma_watch_ticks(uint64_t out[12]);      /* profiling aid: 10 ns ticks of the watchers' drains (arrival found, drain done) */
int grdma_rx_express_ticks(uint64_t out[9]);  /* profiling aid: phase ticks of the express drain (latency engine) */
int grdma_tx_fast_sends(uint64_t out[2]);  /* Sends of streaming jobs planned by k_tx_fast [0], left to the general planner [1] (csrc/grdma_tx_fast.h) */
int grdma_rx_fast_drains(uint64_t out[6]);  /* drains of streaming jobs taken by k_rx_fast [0], declined by reason [1..5] (csrc/grdma_rx_fast.h) */
int grdma_rx_table_cache_stats(uint64_t out[2]);  /* committed drains of the multi-workgroup planner whose read-state tables came out of the connection's table cache [0] / were computed and written back [1] (csrc/grdma_rx_multi.h) */
int grdma_rx_verdict_counts(uint64_t out[2]);  /* drains of the multi-workgroup planner handed to the general planner with a mixed verdict (some workgroups' probes passed, some declined) [0] / with every workgroup declining [1] */
int grdma_debug_set_promise_wait(uint32_t v);  /* test knob: v > 0 makes the promised-credit wait of every other Send workgroup run out after v - 1 polls (0 = the default bound for all) */
uint64_t grdma_wire_wait_runouts(void);  /* fused wire: drain workgroups whose wait for the wire workgroups of their launch ran out (must stay 0) */
int grdma_tx_promise_counts(uint64_t out[4]);  /* promised-credit Sends: priced with it [0], none in the drain [1], an older block [2]; waits that ran out [3] */
int grdma_tx_small_ticks(uint64_t out[8]);  /* profiling aid: phase ticks of the latency engine's small Sends */
/* Scalar ring arithmetic of the host layer (ring_buffer.h:101-143), exported so that the
 * CPU tests can pin it against the oracle without a device. */
uint64_t grdma_host_free_size(uint64_t cap, uint64_t head, uint64_t tail);
uint64_t grdma_host_writable(uint64_t cap, uint64_t head, uint64_t tail);
uint64_t grdma_host_encoded_size(uint64_t payload);
uint64_t grdma_host_calc_writable(uint64_t space);

/* ---- HTTP/2 DATA framing / deframing on the device --------------------------------- */
typedef struct grdma_h2_msg {     /* one gRPC message queued on a stream              */
  const void* payload;            /* serialized message bytes (device-accessible)     */
  uint64_t len;
  uint32_t stream_id;
  uint32_t flags;                 /* 1 = compressed (GRPC_WRITE_INTERNAL_COMPRESS), 2 = END_STREAM */
} grdma_h2_msg;
/* The 5-byte message header (chttp2_transport.cc:1502-1510) + grpc_chttp2_encode_data
 * (frame_data.cc:64-90) for a batch of messages, each sent alone on its stream with
 * open flow-control windows: writes into device memory the slice list
 * grpc_endpoint_write would receive (9-byte frame headers and the 5-byte message
 * header as inlined slices in d_hdr_arena, 32 bytes per slice; payload by
 * reference).  Returns the slice count. */
int64_t grdma_h2_frame_messages(const grdma_h2_msg* msgs, uint64_t n, uint32_t max_frame,
                                grdma_slice* d_slices_out, uint64_t slices_cap,
                                void* d_hdr_arena, uint64_t hdr_cap, uint64_t* wire_bytes);

typedef struct grdma_h2_event {   /* what the deframer saw, in order                  */
  uint32_t kind;                  /* 1 FRAME 2 PAYLOAD 3 MSG_BEGIN 4 MSG_BYTES 5 MSG_END
                                     6 STREAM_OPEN 7 STREAM_CLOSED                       */
  uint32_t a, b, c, d;            /* FRAME: type, flags|status<<8, stream, size         */
                                  /* PAYLOAD: offset in slice, length, is_last          */
                                  /* MSG_BEGIN: compressed, length, stream              */
                                  /* MSG_BYTES: offset in slice, length, stream         */
                                  /* STREAM_OPEN: -, -, stream (accepted from HEADERS)  */
                                  /* STREAM_CLOSED: 1 = left the map / 0 = reads closed, -, stream */
  uint32_t slice;                 /* index of the delivered slice                       */
} grdma_h2_event;
/* connection errors of grpc_chttp2_perform_read (sticky; *h2_error of grdma_h2_deframe) */
enum grdma_h2_error {
  GRDMA_H2_OK = 0,
  GRDMA_H2_ERR_PREFIX = 1,                 /* parsing.cc:91-104  connect string mismatch    */
  GRDMA_H2_ERR_FRAME_TOO_LARGE = 2,        /* parsing.cc:195-205                            */
  GRDMA_H2_ERR_EXPECTED_CONTINUATION = 5,  /* parsing.cc:266-272                            */
  GRDMA_H2_ERR_CONTINUATION_STREAM = 6,    /* parsing.cc:273-281                            */
  GRDMA_H2_ERR_UNEXPECTED_CONTINUATION = 7,/* parsing.cc:287-289                            */
  GRDMA_H2_ERR_FIRST_FRAME = 8,            /* parsing.cc:256-263 first frame must be SETTINGS */
  GRDMA_H2_ERR_MAX_STREAMS = 9,            /* parsing.cc:623-627 (or the stream table is half full) */
  GRDMA_H2_ERR_RST_LENGTH = 10,            /* frame_rst_stream.cc:73-79                     */
  /* malformed control frames (the begin_frame checks of the control-frame parsers): connection errors */
  GRDMA_H2_ERR_SETTINGS_STREAM = 11,       /* parsing.cc:735-739  SETTINGS on a stream      */
  GRDMA_H2_ERR_SETTINGS_ACK_LENGTH = 12,   /* frame_settings.cc:95-101 non-empty ack        */
  GRDMA_H2_ERR_SETTINGS_FLAGS = 13,        /* frame_settings.cc:102-104                     */
  GRDMA_H2_ERR_SETTINGS_LENGTH = 14,       /* frame_settings.cc:105-107 not a multiple of 6 */
  GRDMA_H2_ERR_PING = 15,                  /* frame_ping.cc:58-64 length != 8 or flags      */
  GRDMA_H2_ERR_WINDOW_UPDATE = 16,         /* frame_window_update.cc:56-63                  */
  GRDMA_H2_ERR_GOAWAY = 17,                /* frame_goaway.cc:39-44 shorter than 8 bytes    */
  GRDMA_H2_ERR_TOO_MANY_TRAILERS = 18      /* hpack_parser.cc:1756-1759 third header block without END_HEADERS */
};
enum grdma_h2_parser_flags {
  GRDMA_H2_SERVER = 1,       /* expects the client preface; accepts streams from HEADERS frames
                                (init_header_frame_parser, parsing.cc:596-631)               */
  GRDMA_H2_FIRST_FRAME = 2,  /* fresh connection: the first frame must be SETTINGS           */
  GRDMA_H2_BOUNDARY_STEP = 4,    /* the slice in which a message starts (closing frame of the previous
                                    message + first frame + 5-byte message header, all inside the staged
                                    32 bytes) is parsed in one wave-uniform step instead of byte-wise   */
  GRDMA_H2_NO_BOUNDARY_STEP = 8, /* never; with neither flag the step is on unless the environment
                                    says GRDMA_H2_BOUNDARY_STEP=0                                    */
  GRDMA_H2_BULK_PAIRS = 16,      /* the bulk step gives EVERY lane a frame (lane i: slices s + 2i, s + 2i + 1):
                                    64 frames and 128 slices per step instead of 32 / 64.  On by default since
                                    round 3 (two hardware rounds: 155.7 vs 148.5 and 172.9 vs 155.1 GiB/s in the
                                    with-h2 leg, same events); GRDMA_H2_BULK_PAIRS=0 in the environment or
                                    GRDMA_H2_NO_BULK_PAIRS turns it off                                 */
  GRDMA_H2_NO_BULK_PAIRS = 64,   /* 32 frames per bulk step                                             */
  GRDMA_H2_NO_CHUNKS = 128,      /* always the sequential deframer.  Without it a list of >= 2048 slices is cut at slices in
                                    which a message starts (GRDMA_H2_CHUNKS chunks of >= 128 slices, default 256), the chunks are parsed side
                                    by side and merged when every chunk ended in the state the next one was assumed to
                                    start in -- the sequential deframer does the call otherwise (csrc/grdma_h2_kernels.h) */
  GRDMA_H2_TICKS = 32            /* the parsing wave samples the device clock around its phases (the tick counters
                                    of grdma_h2_pipe_sync / grdma_h2_last_deframe_stats); off by default: a sample
                                    is a scalar memory operation the wave waits for                     */
};
typedef struct grdma_h2_parser grdma_h2_parser;
/* Deframe state of one transport (grpc_chttp2_transport deframe_state & co., internal.h) and
 * its stream map (grpc_chttp2_stream_map) with each stream's grpc_chttp2_data_parser, kept in
 * device memory.  DATA frames are looked up in the map and never create a stream
 * (init_data_frame_parser, parsing.cc:352-374): unknown and read-closed streams are skipped.
 * A server learns its streams from HEADERS frames; a client's streams are opened by the caller
 * when it starts a call.  END_STREAM (on DATA, or on the header block) closes the read side;
 * RST_STREAM closes both; a stream leaves the map once both sides are closed
 * (grpc_chttp2_mark_stream_closed, chttp2_transport.cc:2194-2244) -- the caller reports the write
 * side with grdma_h2_parser_close_writes.  HPACK, SETTINGS, PING, GOAWAY and WINDOW_UPDATE payloads
 * are control plane and are skipped here.  The deframer skips INCOMING WINDOW_UPDATE and SETTINGS payloads too; the send
 * windows (grdma_h2_sw below) read them from the arena by the deframer's events, as the header decoder (grdma_h2_hpack
 * below) reads the HPACK blocks.  Our own WINDOW_UPDATE frames -- the
 * credit for the DATA bytes received -- are produced on the device by the window ledger (grdma_h2_fc below).
 * grdma_h2_parser_create(prefix, max) = create_ex(prefix ? SERVER | FIRST_FRAME : 0, max, 0xffffffff, 0).
 * table_slots: power of two >= 16 (0 = 4096); at most table_slots / 2 streams are live at once. */
grdma_h2_parser* grdma_h2_parser_create(int expect_client_prefix, uint32_t max_frame_size);
grdma_h2_parser* grdma_h2_parser_create_ex(int flags, uint32_t max_frame_size,
                                           uint32_t max_concurrent_streams, uint32_t table_slots);
void grdma_h2_parser_destroy(grdma_h2_parser* p);
/* Batched stream-map updates from the surface; return the number of ids that failed
 * (duplicate / unknown / table full), or <0. */
int grdma_h2_parser_open_streams(grdma_h2_parser* p, const uint32_t* ids, uint32_t n);
int grdma_h2_parser_close_writes(grdma_h2_parser* p, const uint32_t* ids, uint32_t n);
int64_t grdma_h2_parser_live_streams(grdma_h2_parser* p);
/* Duration of the framing / deframing kernel of the last call (HIP events), microseconds. */
double grdma_h2_last_kernel_us(void);
/* Message starts the last grdma_h2_deframe call parsed with the boundary step. */
uint64_t grdma_h2_last_boundary_steps(void);
/* Counters of the last grdma_h2_deframe call: {bulk steps, frames parsed in bulk steps, boundary steps,
 * then device-clock ticks: waiting for staged windows, in bulk steps, in boundary steps, in the
 * byte-wise path, total}. */
void grdma_h2_last_deframe_stats(uint64_t out[8]);
/* The deframer over chunks (lists of >= 2048 slices, unless GRDMA_H2_NO_CHUNKS): out = {calls planned over chunks,
 * calls whose chunks verified and were merged}; the difference went through the sequential deframer. */
int grdma_h2_parser_chunk_stats(grdma_h2_parser* p, uint64_t out[2]);
/* profiling aid: device-clock phase stamps of the last chunked call, 8 words per chunk + 8 of the merge */
int grdma_h2_parser_chunk_dbg(grdma_h2_parser* p, uint64_t* out, uint64_t cap_words);
/* grpc_chttp2_perform_read (parsing.cc:56-253) + grpc_deframe_unprocessed_incoming_frames
 * (frame_data.cc:92-276) over n delivered slices {offset, length} of d_arena.
 * Returns the number of events; *h2_error = connection error, if any. */
int64_t grdma_h2_deframe(grdma_h2_parser* p, const void* d_arena, const grdma_read_slice* slices,
                         uint64_t n, grdma_h2_event* events_out, uint64_t cap, int* h2_error);

/* The delivered slices of MANY transports in one launch (k_h2_deframe_links: one workgroup per item): what a pollset
 * of many connections hands over at once.  Per item the events, the parser state and the stream map are exactly those
 * of grdma_h2_deframe on that item alone; a connection error, an event overflow or an empty list (n == 0) of one item
 * leaves the others untouched, and every item reports for itself (n_events, h2_error).  One upload, one launch, one
 * download -- of every item's whole event capacity, so give tight caps.  Always the sequential deframer per transport
 * (the chunked one stays a single-transport path).  Not thread-safe: one call at a time per process (the call owns a
 * process-wide device block, and the grdma_h2_* calls share one stream).  A parser belongs to one user at a time: while
 * a pipe runs an assembler behind it, the pipe's steps own its state and the batch refuses it; a parser listed in a
 * pipe or group pipe without assembler may be used here between steps (the call is ordered behind the last step).
 * Returns 0, or -GRDMA_ERR_INVALID (nothing ran): n_items outside 1 .. GRDMA_H2_BATCH_MAX, an item without parser or
 * arena, slices NULL with n > 0, events_out NULL with cap > 0, the same parser twice, a parser whose assembler is
 * attached to a pipe. */
#define GRDMA_H2_BATCH_MAX 256
typedef struct grdma_h2_deframe_item {
  grdma_h2_parser* parser;          /* distinct per item */
  const void* d_arena;              /* the arena this transport's slices point into */
  const grdma_read_slice* slices;   /* host array, as grdma_h2_deframe takes it */
  uint64_t n;
  grdma_h2_event* events_out;       /* host, may be NULL (then cap = 0) */
  uint64_t cap;
  int64_t n_events;                 /* out: events, or -GRDMA_ERR_CAPACITY for this item */
  int h2_error;                     /* out: this transport's connection error */
} grdma_h2_deframe_item;
int grdma_h2_deframe_batch(grdma_h2_deframe_item* items, uint32_t n_items);

/* HTTP/2 inside the device pipeline: per step, k_h2_frame_index + k_h2_frame_emit rebuild the slice list of the job's
 * link from the message table (grpc_chttp2_encode_data, frame_data.cc:64-90), the streaming job
 * carries it through the connection, and k_h2_deframe parses the slices the job delivered
 * (grpc_chttp2_perform_read + grpc_deframe_unprocessed_incoming_frames) -- three stages on three
 * streams ordered by events, nothing returns to the host in between.  The job must have been run
 * once (graph captured / engine prepared); delivered_slices is what that run delivered.  Two pipes
 * over two jobs of one connection may alternate: framing and deframing then run beside the other
 * job's step.  schedule: 0 = the job's graph (the only one). */
typedef struct grdma_h2_pipe grdma_h2_pipe;
grdma_h2_pipe* grdma_h2_pipe_create(grdma_stream_job* job, uint32_t link, const grdma_h2_msg* msgs, uint64_t nmsgs,
                                    uint32_t max_frame, grdma_h2_parser* parser, uint64_t delivered_slices,
                                    uint64_t events_cap);
int grdma_h2_pipe_enqueue(grdma_h2_pipe* p, int schedule);
/* out = {slices framed, frame overflow, events, deframe overflow, slices parsed, h2 error,
 *        framing kernel us, deframing kernel us (of the last step), bulk steps of the deframer,
 *        frames it parsed in bulk steps, and four profiling tick counts of the deframer: waiting for
 *        staged windows, inside bulk steps, total, inside the byte-wise path} */
int grdma_h2_pipe_sync(grdma_h2_pipe* p, uint64_t out[14], grdma_h2_event* events_out, uint64_t cap);
void grdma_h2_pipe_destroy(grdma_h2_pipe* p);
/* out = {message starts the last synced step parsed with the boundary step, device-clock ticks inside it} */
int grdma_h2_pipe_boundary_stats(grdma_h2_pipe* p, uint64_t out[2]);

/* ---- Received gRPC messages in device memory (the message assembler, csrc/grdma_h2_asm.h) ----
 * Behind the deframer of one parser, on the device: every message's payload is copied out of the receive arena into a
 * ring over d_arena (contiguous, 256-byte granules) and described by one grdma_h2_rx_msg, in the order of the events
 * that finish the messages (MSG_END, or STREAM_CLOSED / a connection error while the message is partial).  The
 * surface's receive_message gets its grpc_byte_buffer this way (call.cc receiving_slice_ready /
 * continue_receiving_slices); max_message_bytes is the message_size filter's limit (0 = none). */
typedef struct grdma_h2_rx_msg {
  uint64_t offset;                /* in d_arena (0 unless OK)                                    */
  uint64_t length;                /* from the 5-byte message header                              */
  uint64_t seq;                   /* the message's MSG_BEGIN number on this assembler            */
  uint32_t stream_id, status, flags, pad;  /* flags bit 0: compressed (passed through)           */
} grdma_h2_rx_msg;
enum grdma_h2_msg_status {
  GRDMA_H2_MSG_OK = 0,
  GRDMA_H2_MSG_TOO_LARGE = 1,     /* length > max_message_bytes: its bytes are dropped           */
  GRDMA_H2_MSG_NO_SPACE = 2,      /* the ring (or max_pending) was full at its MSG_BEGIN         */
  GRDMA_H2_MSG_TRUNCATED = 3      /* its stream closed, or the connection failed, mid-message    */
};
typedef struct grdma_h2_asm grdma_h2_asm;
grdma_h2_asm* grdma_h2_asm_create(grdma_h2_parser* parser, void* d_arena, uint64_t arena_bytes,
                                  uint64_t max_message_bytes, uint32_t max_pending);
void grdma_h2_asm_destroy(grdma_h2_asm* a);   /* does nothing while a pipe has it attached: destroy the pipes first */
/* grdma_h2_deframe + the assembler; returns the number of descriptors written to msgs_out.  events_out may be NULL
 * (no event copy; ev_cap still sizes the device's event list).  -GRDMA_ERR_CAPACITY when events or descriptors
 * overflow their caps; -GRDMA_ERR_INVALID for bad arguments or an assembler attached to a pipe.
 * A call plans at most 3072 distinct streams with message events.  One with more fails with -GRDMA_ERR_CAPACITY and
 * assembles NOTHING: no descriptor, no byte of the arena, and the ring, its records, the reported count and the seq
 * counter stay as they were (the call after it numbers its messages where the call before it stopped).  The deframer
 * has consumed the bytes all the same (events_out and *h2_error are valid): the messages of the failed call are lost,
 * and a message a stream carried into it is dropped -- its space is given back at the next release, no descriptor ever
 * reports it, later bytes of it are ignored.  The same holds per item of grdma_h2_deframe_messages_batch and per step
 * of a pipe (whose release of the earlier messages has happened by then). */
int64_t grdma_h2_deframe_messages(grdma_h2_parser* p, grdma_h2_asm* a, const void* d_arena,
                                  const grdma_read_slice* slices, uint64_t n,
                                  grdma_h2_event* events_out, uint64_t ev_cap,
                                  grdma_h2_rx_msg* msgs_out, uint64_t msgs_cap, int* h2_error);
/* release the oldest `count` reported messages not yet released (ordered on the device after earlier work);
 * -GRDMA_ERR_INVALID on an assembler attached to a pipe (each pipe step releases everything reported before it) */
int grdma_h2_asm_release(grdma_h2_asm* a, uint64_t count);
/* out = {reported, OK bytes, too large, no space, truncated (since creation), bytes in use,
 *        plan us, copy us (of the last standalone call; 0 in a fused pipe)} */
int grdma_h2_asm_stats(grdma_h2_asm* a, uint64_t out[8]);
/* every later step of the pipe assembles its messages (first releasing all reported before); a's parser must be the
 * pipe's.  Several pipes of one parser share its assembler. */
int grdma_h2_pipe_attach_assembler(grdma_h2_pipe* p, grdma_h2_asm* a);
/* the descriptors of the last synced step: their number, or -GRDMA_ERR_CAPACITY if more than cap */
int64_t grdma_h2_pipe_messages(grdma_h2_pipe* p, grdma_h2_rx_msg* out, uint64_t cap);

/* grdma_h2_deframe_messages for MANY transports at once (k_h2_deframe_links, then the six k_h2_asm_*_links kernels over
 * a table of the items' assemblers): seven launches for any n_items, the one-workgroup stages of the plan side by side.
 * An item is a grdma_h2_deframe_item plus its assembler and descriptor array; cap sizes the device's event list
 * (>= 1) and events_out may be NULL, as in the single call.  Per item the report is what grdma_h2_deframe_messages
 * reports for that transport alone: h2_error, n_events (-GRDMA_ERR_CAPACITY on an event overflow), the events if asked
 * for, n_msgs (-GRDMA_ERR_CAPACITY on an event overflow, more streams than a call plans, more descriptors than
 * msgs_cap) and the descriptors.  Nothing is shared between the items: an overflow, NO_SPACE or a connection error of
 * one leaves the others' descriptors and bytes what they would be alone.  One upload and one download of results and
 * events; the descriptors come from each assembler's own buffer.  Ordered behind each parser's last pipe step; one call
 * at a time per process, as grdma_h2_deframe_batch.
 * Returns 0, or -GRDMA_ERR_INVALID (nothing ran, grdma_last_error says why): n_items outside 1 .. GRDMA_H2_BATCH_MAX,
 * an item without parser, arena, assembler or event capacity, slices NULL with n > 0, msgs_out NULL with msgs_cap > 0,
 * an assembler whose parser is not the item's, a parser or an assembler listed twice, an assembler attached to a pipe
 * or group pipe. */
typedef struct grdma_h2_messages_item {
  grdma_h2_parser* parser;          /* distinct per item */
  const void* d_arena;              /* the arena this transport's slices point into */
  const grdma_read_slice* slices;   /* host array */
  uint64_t n;
  grdma_h2_event* events_out;       /* host, may be NULL: no event copy */
  uint64_t cap;                     /* events the device's list holds, >= 1 */
  int64_t n_events;                 /* out: events, or -GRDMA_ERR_CAPACITY for this item */
  int h2_error;                     /* out: this transport's connection error */
  grdma_h2_asm* assembler;          /* of `parser`; distinct per item */
  grdma_h2_rx_msg* msgs_out;        /* host */
  uint64_t msgs_cap;
  int64_t n_msgs;                   /* out: descriptors, or -GRDMA_ERR_CAPACITY for this item */
} grdma_h2_messages_item;
int grdma_h2_deframe_messages_batch(grdma_h2_messages_item* items, uint32_t n_items);
/* grdma_h2_asm_release for n assemblers in ONE launch (k_h2_asm_release_links): entry i releases the oldest counts[i]
 * reported messages of asms[i].  -GRDMA_ERR_INVALID (nothing released): n outside 1 .. GRDMA_H2_BATCH_MAX, a NULL
 * entry, an assembler listed twice or attached to a pipe or group pipe. */
int grdma_h2_asm_release_batch(grdma_h2_asm* const* asms, const uint64_t* counts, uint32_t n);

/* ---- Replies framed on the device from received-message descriptors (csrc/grdma_h2_reply.h) ----
 * What a data plane does with a received message without looking inside it: send it back (echo) or on to another
 * stream (a proxy).  The descriptors of the source assembler's LAST call are framed where they lie: the wire is what
 * grdma_h2_frame_messages yields for the kept messages in reported order (compressed flag passed through, never
 * END_STREAM, open flow-control windows).  Kept: status GRDMA_H2_MSG_OK only (the others own no bytes), and
 *   - without a route table (routes NULL or n_routes 0): every message, on the stream it came in on;
 *   - with one (at most 4096 entries, sorted by the library): a message whose stream is a from_stream goes out on
 *     its to_stream, any other is dropped and counted as unrouted.  A duplicate from_stream or a zero id: NULL.
 * Payload goes by reference: the slices point into the assembler's arena, so the messages must stay unreleased until
 * the send that gathers them is done -- grdma_h2_asm_release is the caller's to order behind it. */
typedef struct grdma_h2_route { uint32_t from_stream, to_stream; } grdma_h2_route;
typedef struct grdma_h2_reply grdma_h2_reply;   /* route table + scratch for up to max_messages descriptors */
grdma_h2_reply* grdma_h2_reply_create(grdma_h2_asm* source, const grdma_h2_route* routes, uint32_t n_routes,
                                      uint32_t max_frame, uint64_t max_messages);
/* does nothing while a reply pipe frames through it: destroy the pipe first.  Destroy the reply before its source. */
void grdma_h2_reply_destroy(grdma_h2_reply* r);
/* Frames what the source assembler's last grdma_h2_deframe_messages reported (ordered behind it on the device);
 * returns the slice count.  out = {kept, dropped by status, dropped as unrouted, slices, header-arena bytes, wire
 * bytes, overflow, framing time in microseconds (HIP events)}.  -GRDMA_ERR_CAPACITY when the slices or the header
 * arena (32 bytes per inlined slice, 16-byte aligned) overflow their caps or the call reported more than max_messages
 * descriptors: nothing is written then.  -GRDMA_ERR_INVALID for null, zero or misaligned arguments and for a source
 * attached to a pipe (grdma_h2_pipe_create_reply frames that one). */
int64_t grdma_h2_reply_frame(grdma_h2_reply* r, grdma_slice* d_slices_out, uint64_t slices_cap,
                             void* d_hdr_arena, uint64_t hdr_cap, uint64_t out[8]);
/* grdma_h2_reply_frame for MANY transports at once (k_h2_reply_plan_links, k_h2_reply_emit_links over a table of the
 * items' framers): two launches for any n_items, the one-workgroup plans side by side, the messages of all items laid
 * out by one grid.  One upload of the table and the per-item targets, one download of the result blocks; ordered
 * behind each source parser's last deframing.  Per item the report (out[0..6], n_slices) and the bytes written are
 * exactly what grdma_h2_reply_frame gives for that reply alone; out[7] is the batch's framing time, repeated.  Nothing
 * is shared between the items: an item whose slices or header arena overflow its caps, whose call reported more than
 * max_messages descriptors or whose source skipped its last call gets n_slices = -GRDMA_ERR_CAPACITY and nothing of it
 * is written; the others are framed as they would be alone.  One call at a time per process, as grdma_h2_deframe_batch.
 * Returns 0, or -GRDMA_ERR_INVALID (nothing ran, grdma_last_error says why): n_items outside 1 .. GRDMA_H2_BATCH_MAX,
 * a NULL reply, a reply listed twice, two replies of one source assembler (one item per transport), a null, zero or
 * misaligned slice table or header arena (as in the single call), a source attached to a pipe or group pipe, a reply
 * bound to a reply pipe. */
typedef struct grdma_h2_reply_item {
  grdma_h2_reply* reply;            /* distinct; its source assembler distinct and not attached to a pipe */
  grdma_slice* d_slices_out;        /* device, 16-byte aligned */
  uint64_t slices_cap;
  void* d_hdr_arena;                /* device, 16-byte aligned */
  uint64_t hdr_cap;
  uint64_t out[8];                  /* the words of grdma_h2_reply_frame; out[7] is the batch's time, repeated */
  int64_t n_slices;                 /* out: slice count, or -GRDMA_ERR_CAPACITY for this item alone */
} grdma_h2_reply_item;
int grdma_h2_reply_frame_batch(grdma_h2_reply_item* items, uint32_t n_items);
/* A pipe whose framing stage is the reply: a step frames what the LAST ENQUEUED step of the forward pipes (the pipes
 * `reply`'s source assembler is attached to) reported, sends it through job_back and deframes it with parser_back.
 * Everything else is grdma_h2_pipe: enqueue, sync, attach_assembler, messages, destroy.  job_back has run once over a
 * slice list of the lengths the reply will have; recorded_wire_bytes is what that run sent
 * (grdma_stream_result::bytes_sent).  A step whose reply has another slice count or other wire bytes writes nothing:
 * the job re-sends its previous table, and grdma_h2_pipe_sync reports frame overflow = 2.  Ordering is by events: the
 * step waits for the forward step's assembler, and a forward step's release waits for the last reply step that read
 * the arena.  Destroy the reply pipe before the forward pipes (their destroy does nothing while it exists) and
 * before `reply`. */
grdma_h2_pipe* grdma_h2_pipe_create_reply(grdma_stream_job* job_back, uint32_t link, grdma_h2_reply* reply,
                                          grdma_h2_parser* parser_back, uint64_t delivered_slices, uint64_t events_cap,
                                          uint64_t recorded_wire_bytes);
/* the slice table the pipe's job sends from (what the framing stage last wrote), after the enqueued steps have ended:
 * the number of entries, or -GRDMA_ERR_CAPACITY if more than cap */
int64_t grdma_h2_pipe_slice_table(grdma_h2_pipe* p, grdma_slice* out, uint64_t cap);

/* ---- Receive flow control on the device: the window ledger (csrc/grdma_h2_fc.h) ----
 * The receive half of RFC 7540 6.9 for one transport: the DATA bytes of one deframing are counted against the windows
 * our SETTINGS announced, and the WINDOW_UPDATE frames that return them are written on the device.  A fixed policy
 * with the counting position of the reference's RecvData (init_data_frame_parser), not a port of flow_control.cc (no
 * BDP estimate).  Input: the device event list of one deframing of the ledger's parser.
 *  1. Connection.  Every DATA frame of the call counts with its whole frame size at its FRAME event, whatever its
 *     stream (frames the deframer skips included; a frame whose payload continues in the next call counts once, in
 *     the call that saw its header).  D = the call's sum.  D above the announced window: GRDMA_H2_FC_CONN_OVERFLOW.
 *     The window goes down by D.  pending = conn_window - announced; pending > 0 and >= conn_threshold: one
 *     WINDOW_UPDATE(stream 0, pending) and the announced window is conn_window again.
 *  2. Streams are stateless across calls.  S = a stream's sum over the DATA frames DELIVERED to its data parser in
 *     this call: status 0, in front of the stream's first STREAM_CLOSED event and, for a stream the call opened,
 *     behind its STREAM_OPEN; a stream with neither event counts only if the parser's stream map holds it open for
 *     reads (the deframer skips unknown and read-closed streams without saying so in the event).  S > stream_window:
 *     GRDMA_H2_FC_STREAM_OVERFLOW, counted per stream, the first such stream (by its first counted frame) reported.
 *     S > 0 and no STREAM_CLOSED event in the call: one WINDOW_UPDATE(stream, S).  A closed stream gets none; its
 *     bytes counted for the connection.  (A stream whose reads were closed in an EARLIER call and that this call's
 *     RST_STREAM removes is taken as open in front of that event: it gets no frame either way, only the violation
 *     count can see its skipped bytes.)  An increment above 2^31 - 1 is cut to that.
 *  3. Order: the connection's frame, then the streams in the order of their first counted DATA frame.
 *  4. A call that ended with a connection error accounts and emits nothing.  A call whose event list overflowed (or
 *     in which more streams were live, opened or closed than the stream map has slots) cannot be accounted: the sticky GRDMA_H2_FC_LOST flag
 *     (in this and every later result block), -GRDMA_ERR_CAPACITY, overflow word 2, nothing else changes.  More than
 *     max_updates frames, or a slice or header cap too small: overflow word 1, nothing is written, the window state
 *     advances and the result block keeps the totals, so the caller sees what was not sent.
 * Output: 13-byte frames (frame_window_update.cc) in a header arena, 32 bytes of arena per slice, as the slice list
 * grpc_slice_buffer_add builds from them: the concatenated frames cut into 23-byte inlined slices, the last one
 * shorter.  The list is an outbuf of its own: nothing merges across its end into what the caller sends behind it.
 * Result block: {frames, slices, wire bytes, connection bytes counted, stream bytes credited, violations
 * (GRDMA_H2_FC_*), first violating stream, overflow}.
 * Many links: grdma_h2_fc_account_batch and grdma_h2_group_pipe_attach_flow_control below.
 * Not here: ledgers in the batch deframers (grdma_h2_deframe_batch and grdma_h2_deframe_messages_batch refuse a parser
 * that has a ledger) and the frames inside a reply pipe's slice table.  The send half -- the peer's windows and a framer
 * under them -- is grdma_h2_sw below; the other framers (grdma_h2_frame_messages, the pipes, grdma_h2_reply_*) still do
 * not look at the peer's windows. */
enum grdma_h2_fc_violation { GRDMA_H2_FC_CONN_OVERFLOW = 1, GRDMA_H2_FC_STREAM_OVERFLOW = 2, GRDMA_H2_FC_LOST = 4 };
typedef struct grdma_h2_fc grdma_h2_fc;
/* stream_window 1 .. 2^31-1 (what SETTINGS announced per stream), conn_window 65535 .. 2^31-1 (kept announced),
 * conn_threshold 0 .. conn_window, max_updates 1 .. 2^24 (frames of one call).  One ledger per parser: NULL for a
 * second one (grdma_last_error says why). */
grdma_h2_fc* grdma_h2_fc_create(grdma_h2_parser* parser, uint32_t stream_window, uint32_t conn_window,
                                uint32_t conn_threshold, uint32_t max_updates);
/* does nothing while a pipe has the ledger attached: destroy the pipe first.  A ledger whose parser was destroyed
 * first refuses every call (-GRDMA_ERR_INVALID) and can still be destroyed. */
void grdma_h2_fc_destroy(grdma_h2_fc* fc);
/* Accounts the LAST standalone deframing of the ledger's parser (grdma_h2_deframe or grdma_h2_deframe_messages),
 * ordered behind it on the device (and behind the parser's last pipe step); call it before the stream map is changed,
 * from the host or by a pipe step of the same parser: rule 2 looks streams up in the map as it is then.  Returns the slice count;
 * out = the result block.  -GRDMA_ERR_INVALID (grdma_last_error says why): the same call accounted twice, no call yet,
 * a ledger attached to a pipe, null, zero or misaligned (16 bytes) targets.  -GRDMA_ERR_CAPACITY: rule 4 (out is set). */
int64_t grdma_h2_fc_account(grdma_h2_fc* fc, grdma_slice* d_slices_out, uint64_t slices_cap, void* d_hdr_arena,
                            uint64_t hdr_cap, uint64_t out[8]);
/* {calls accounted, connection bytes, stream bytes credited, frames emitted, connection overflows (calls), stream
 * overflows (streams; bit 63: the LOST flag), the announced connection window (int64), kernel time of the last
 * standalone call in NANOseconds (HIP events)} */
int grdma_h2_fc_stats(grdma_h2_fc* fc, uint64_t out[8]);
/* The ledger's five kernels become part of every step of a forward grdma_h2_pipe: behind the deframer, in attach order
 * with the assembler's (it reads the events only, either order gives the same bytes).  Fused they are nodes of the
 * job's graph (grdma_job_hook_counts' second word grows by 5), with GRDMA_H2_PIPE_FUSED=0 they are enqueued behind the
 * deframer.  The pipe owns the output tables (room for max_updates frames).  -GRDMA_ERR_INVALID: the ledger of another
 * parser, a reply pipe, a second attach, a ledger attached elsewhere. */
int grdma_h2_pipe_attach_flow_control(grdma_h2_pipe* pipe, grdma_h2_fc* fc);
/* the window-update list of the last step, after the enqueued steps have ended: the slice count and the result block */
int64_t grdma_h2_pipe_window_updates(grdma_h2_pipe* pipe, grdma_slice* slices_out, uint64_t cap, uint64_t out[8]);
/* ... and its wire image: the number of bytes */
int64_t grdma_h2_pipe_window_update_bytes(grdma_h2_pipe* pipe, void* bytes_out, uint64_t cap);
/* grdma_h2_fc_account for n ledgers (1 .. GRDMA_H2_BATCH_MAX) in the same five launches (k_h2_links_fc_*): every ledger
 * accounts the last standalone deframing of its OWN parser, exactly as the single call does, ordered behind it and behind
 * every parser's last pipe step.  out: 8 result words per item, in item order.  What differs from the single call: an
 * item's overflow (word 7: 1 = a cap, 2 = the call could not be accounted) is reported in its own words only and writes
 * nothing for that item, the other items are exact; the return value is the number of items accounted without
 * overflow, or a negative error.  -GRDMA_ERR_INVALID (nothing runs, grdma_last_error says why): n outside the range, a
 * NULL ledger or one listed twice, a ledger attached to a pipe, a ledger whose parser is gone, has deframed nothing
 * yet or whose last call is accounted already, null, zero or misaligned (16 bytes) targets. */
typedef struct grdma_h2_fc_item {
  grdma_h2_fc* fc;            /* distinct */
  grdma_slice* d_slices_out;  /* device slice table of the item */
  uint64_t slices_cap;
  void* d_hdr_arena;          /* device header arena of the item, 32 bytes per slice */
  uint64_t hdr_cap;
} grdma_h2_fc_item;
int grdma_h2_fc_account_batch(const grdma_h2_fc_item* items, uint32_t n, uint64_t* out);

/* ---- Send flow control on the device: the peer's windows (csrc/grdma_h2_sw.h) ----
 * The send half of RFC 7540 6.9 for one transport.  The peer's windows live in device memory, are fed from the
 * deframer's events (the peer's WINDOW_UPDATE and SETTINGS frames arrive on the parser of the same transport), and
 * grdma_h2_sw_frame never sends a byte the peer has not allowed and carries the rest over.  The sending rule is the
 * reference's DataSendContext::max_outgoing (writing.cc): min(peer MAX_FRAME_SIZE, stream window, connection window),
 * a stream's window being peer INITIAL_WINDOW_SIZE + delta (delta = credit received - bytes sent; a SETTINGS change is
 * one scalar).  A fixed policy, not a port of flow_control.cc.
 * INTAKE (grdma_h2_sw_intake) takes in the LAST standalone deframing of the parser (grdma_h2_deframe or
 * grdma_h2_deframe_messages): its device event list, its slice table and its receive arena, which must still hold the
 * call's bytes.  It is ordered behind that call on the device; call it before the stream map is changed from the host.
 *  1. A frame's payload is the run of PAYLOAD events behind its FRAME event; PAYLOAD events in front of the call's
 *     first FRAME event continue the frame the previous call's end cut (the carry: at most 3 bytes of a WINDOW_UPDATE
 *     or 5 of a SETTINGS entry, plus the values of the unfinished SETTINGS frame).
 *  2. WINDOW_UPDATE: the increment is the 4 payload bytes.  0, or bit 31 set: GRDMA_H2_SW_BAD_INCREMENT, nothing is
 *     added.  Stream 0 adds to the connection's window; another id adds to its stream's delta iff the parser's map
 *     holds the stream -- judged at the END of the call, not at the frame, which differs only for a stream that opens
 *     or leaves inside the call; otherwise the frame is ignored, as the reference ignores a stream it cannot look up.
 *     A window that would pass 2^31 - 1 stays there (GRDMA_H2_SW_WINDOW_OVERFLOW); the call's sum is judged, with the
 *     INITIAL_WINDOW_SIZE the call leaves, for the connection and the streams that got credit in the call.
 *  3. SETTINGS (not an ACK): entries of 6 bytes, id 4 = INITIAL_WINDOW_SIZE (above 2^31 - 1: GRDMA_H2_SW_BAD_SETTINGS,
 *     not taken), id 5 = MAX_FRAME_SIZE (outside 16384 .. 2^24 - 1: the same), other ids ignored.  The values take effect
 *     when the frame's LAST byte is in (a frame cut by a call's end: in the call that completes it); of several frames
 *     the last wins, value by value.
 *  4. An entry whose stream the map no longer holds at the end of the call is dropped (RST_STREAM, END_STREAM on both
 *     sides, grdma_h2_parser_close_writes); the same id opened again starts at delta 0.
 *  5. A call that ended with a connection error takes nothing in.  A call whose event list overflowed: the sticky
 *     GRDMA_H2_SW_LOST flag, -GRDMA_ERR_CAPACITY, overflow word 2, the carry is dropped, nothing else changes.  A
 *     standalone deframing that was never taken in sets the flag too and drops the carry; the windows keep what they
 *     know and every later result block carries the flag.
 *  Result block: {WINDOW_UPDATE frames applied, connection credit added, stream credit added, SETTINGS frames applied,
 *  violations (GRDMA_H2_SW_*), first offending stream (by event order; 0: the connection or a SETTINGS frame), live
 *  entries, overflow}.  Returns the number of WINDOW_UPDATE frames applied.
 * FRAMING (grdma_h2_sw_frame) is grdma_h2_frame_messages under the windows, for 1 .. 4096 messages.  progress[i] (in/out,
 * host) is how many of message i's 5 + len flow-controlled bytes earlier calls have sent; the caller submits unfinished
 * messages again, the messages of one stream in their order.  r_i = 5 + len_i - progress_i (0 is refused), mf =
 * min(max_frame, peer MAX_FRAME_SIZE).  In table order each message gets min(r_i, its stream's window, the connection's
 * window), and nothing once an earlier message of its stream is unfinished; a stream the map does not hold gets
 * nothing.  (Computed as a_i = min(r_i, max(0, W_s - sum of r_j over earlier messages of s)), g_i = min(a_i, max(0, C -
 * sum of a_j over earlier messages)).)  Message i puts bytes [progress_i, progress_i + g_i) of [5-byte header | payload]
 * into DATA frames of mf bytes, the last one shorter, END_STREAM only on the frame that completes a message flagged so,
 * never a frame of size 0; the slice list is what grpc_slice_buffer_move_first_no_ref and grpc_slice_buffer_add make of
 * it on ONE outbuf per call.  Then delta_s and the connection's window go down by what was granted.  A slice or header
 * cap too small: -GRDMA_ERR_CAPACITY, overflow word 1, the totals in the result block -- and NOTHING is written, no window
 * moves, progress stays (unlike the ledger: these bytes were not sent).  A stream a call names has an entry (delta 0)
 * from then on.  Result block: {messages completed, messages cut or held, slices, header-arena bytes, wire bytes,
 * flow-controlled bytes granted, stall bits (1 = the connection's window, 2 = a stream's, 4 = an unknown stream),
 * overflow}.  Returns the slice count.
 * -GRDMA_ERR_INVALID or NULL (grdma_last_error says why): a second grdma_h2_sw on a parser, windows above 2^31 - 1, intake
 * with no call yet or of the same call twice, a parser that is gone (destroy still works), n = 0 or above 4096, r_i = 0,
 * max_frame 0 or >= 2^24, null, zero or misaligned (16 bytes) targets.
 * Not here: intake of a pipe's or group pipe's steps and the windowed framer as a pipe's framing stage (a job's graph
 * carries a fixed slice count per step; a window-cut step has another shape), the
 * other settings, the HPACK encoder (the decoder: grdma_h2_hpack below) (the reply framer under these windows: grdma_h2_reply_frame_windowed below) (SETTINGS ACK: grdma_h2_ctl below).  (The many-link batch forms: grdma_h2_sw_intake_batch / _frame_batch below.) */
enum grdma_h2_sw_violation { GRDMA_H2_SW_BAD_INCREMENT = 1, GRDMA_H2_SW_WINDOW_OVERFLOW = 2, GRDMA_H2_SW_BAD_SETTINGS = 4,
                             GRDMA_H2_SW_LOST = 8 };
typedef struct grdma_h2_sw grdma_h2_sw;
/* initial_window, conn_window 0 .. 2^31-1 (RFC 7540: 65535 each until the peer says otherwise), peer_max_frame
 * 16384 .. 2^24-1 (16384).  One per parser.  Standalone deframings in front of the creation are not its business. */
grdma_h2_sw* grdma_h2_sw_create(grdma_h2_parser* parser, uint32_t initial_window, uint32_t conn_window, uint32_t peer_max_frame);
void grdma_h2_sw_destroy(grdma_h2_sw* sw);
int64_t grdma_h2_sw_intake(grdma_h2_sw* sw, uint64_t out[8]);
int64_t grdma_h2_sw_frame(grdma_h2_sw* sw, const grdma_h2_msg* msgs, uint64_t* progress, uint64_t n, uint32_t max_frame,
                          grdma_slice* d_slices_out, uint64_t slices_cap, void* d_hdr_arena, uint64_t hdr_cap, uint64_t out[8]);
/* the windows as they are: ids[i] = 0 is the connection's, another id its stream's (INITIAL_WINDOW_SIZE + delta) */
int grdma_h2_sw_windows(grdma_h2_sw* sw, const uint32_t* ids, uint32_t n, int64_t* out);
/* {intakes, WINDOW_UPDATE frames applied, SETTINGS frames applied, violations (bit 63: the LOST flag), framing calls,
 * flow-controlled bytes sent, peer INITIAL_WINDOW_SIZE | peer MAX_FRAME_SIZE << 32, kernel time of the last call in
 * NANOseconds (HIP events)} */
int grdma_h2_sw_stats(grdma_h2_sw* sw, uint64_t out[8]);
/* grdma_h2_sw_intake for n send windows (1 .. GRDMA_H2_BATCH_MAX) in the same three launches (k_h2_links_sw_clear /
 * _take / _finish): every sws[i] takes in the last standalone deframing of its OWN parser, exactly as the single call
 * does (rules 1 .. 5 above, the skipped deframing judged per item), ordered behind it and behind every parser's last
 * pipe step.  out: 8 result words per item, in item order.  What differs from the single call: an item's lost call
 * (sticky GRDMA_H2_SW_LOST, overflow word 2, carry dropped) is reported in its own words only, the other items are
 * exact; the return value is the number of items whose overflow word is 0, or a negative error.  -GRDMA_ERR_INVALID
 * (nothing runs, nothing changes, grdma_last_error says why): n outside the range, a NULL array, a NULL item or one
 * listed twice, an item whose parser is gone, has deframed nothing yet, whose last call is taken in already or whose
 * event capacity is 0xfffffff0 or more (event positions are 32 bits). */
int grdma_h2_sw_intake_batch(grdma_h2_sw* const* sws, uint32_t n, uint64_t* out);
/* grdma_h2_sw_frame for n send windows (1 .. GRDMA_H2_BATCH_MAX) in the same two launches (k_h2_links_sw_plan / _emit):
 * every item frames its own message table under its own windows into its own targets, exactly as the single call does.
 * out: 8 result words per item, in item order.  What differs from the single call: an item whose slice or header cap is
 * too small (overflow word 1) writes nothing, moves no window and keeps its progress, and the other items are framed;
 * the return value is the number of items without overflow, or a negative error.  -GRDMA_ERR_INVALID (nothing runs,
 * nothing changes): n outside the range, a NULL array, an item without send windows or with the same ones as another
 * (two plans would share their tables), a parser that is gone, and per item what grdma_h2_sw_frame refuses: no message
 * table or progress, nmsgs 0 or above 4096, max_frame 0 or >= 2^24, a message of 2^32 bytes or more, progress[i] >= 5 +
 * len, null, zero or misaligned (16 bytes) targets. */
typedef struct grdma_h2_sw_frame_item {
  grdma_h2_sw* sw;            /* distinct */
  const grdma_h2_msg* msgs;   /* host message table of the item */
  uint64_t* progress;         /* in/out, host: as grdma_h2_sw_frame's */
  uint64_t nmsgs;
  uint32_t max_frame;
  uint32_t pad;
  grdma_slice* d_slices_out;  /* device slice table of the item */
  uint64_t slices_cap;
  void* d_hdr_arena;          /* device header arena of the item, 32 bytes per frame */
  uint64_t hdr_cap;
} grdma_h2_sw_frame_item;
int grdma_h2_sw_frame_batch(const grdma_h2_sw_frame_item* items, uint32_t n, uint64_t* out);

/* ---- Replies under the peer's windows (csrc/grdma_h2_wr.h) ----
 * grdma_h2_reply_frame under a grdma_h2_sw: the device-resident reply path (deframer, assembler, reply, wire) against a
 * peer that holds it to its windows.  What the windows cut off waits in a queue in DEVICE memory -- a reply has no host
 * table -- and its bytes stay unreleased in the source assembler's ring until they are sent.
 * BINDING.  grdma_h2_reply_attach_windows(reply, sw, max_pending) binds a reply framer to the send windows of the
 *  transport its replies go OUT on: for an echo the send windows of the source assembler's own parser, for a proxy
 *  another transport's.  It allocates the queue, max_pending = 1 .. 4096 entries (the windowed plan's limit).  One
 *  attachment per reply and one per sw.  Source calls in front of the attachment are not the queue's business.
 *  -GRDMA_ERR_INVALID: a reply bound to a reply pipe, a source assembler attached to a pipe, a second attachment of either,
 *  a sw whose parser is gone.  grdma_h2_reply_destroy and grdma_h2_sw_destroy work in either order; after the other is
 *  gone every call on the survivor but destroy is refused (the queue held what the windows had promised).
 *  grdma_h2_reply_frame on an attached reply is refused: one message could go out twice.
 * THE CALL.  grdma_h2_reply_frame_windowed frames ONE message table: [the queue's entries, in their order | the kept
 *  descriptors of the source assembler's last call, in reported order].  The second part is there only if that call has
 *  not been taken yet and flags lacks GRDMA_H2_WR_PENDING_ONLY.  Kept and routed as grdma_h2_reply_frame keeps and
 *  routes: status OK, the route table, the compressed flag passed through, never END_STREAM.  The table is framed as
 *  grdma_h2_sw_frame frames a host table with the same messages and progress (the grant, the piece layout, mf =
 *  min(the reply's max_frame, peer MAX_FRAME_SIZE), the slice merge rules); new entries start at progress 0.  An entry
 *  that finishes leaves the queue, the others stay in order with their new progress: per-stream order is the queue's
 *  order, and the grant gives nothing once an earlier message of the stream is unfinished.
 * CLOSED STREAMS.  Before the grant every entry, old or new, is looked up in the map of the sw's parser.  An entry whose
 *  outgoing stream the map does not hold is dropped -- even one that is partly sent -- and counted in `dropped closed`:
 *  the peer has reset or finished that stream, and a message that can never be granted must not pin the ring.  So the
 *  stall bits never carry 4 (an unknown stream).
 * TAKING THE SOURCE'S CALLS.  The assembler counts its standalone calls (grdma_h2_deframe_messages and _batch).  A
 *  call taken already and no flag: the queue alone is framed.  No source call since the attachment and an empty queue:
 *  -GRDMA_ERR_INVALID.  A source call that was never taken because the count ran ahead by more than one: the sticky
 *  GRDMA_H2_WR_LOST in the flags word; the call itself is answered.  A call the assembler skipped, or more descriptors
 *  than the reply's max_messages: overflow word 1.
 * OVERFLOW.  A slice or header cap too small: overflow word 1, the totals in their words.  More entries than
 *  max_pending: overflow word 2, their count in the `still pending` word.  Both: -GRDMA_ERR_CAPACITY, NOTHING is
 *  written, no window moves, the queue and its progress stand, the source call is NOT taken, the words 8 .. 11 are 0.
 *  Repeat the call with larger targets, or with GRDMA_H2_WR_PENDING_ONLY once credit has come in.
 * RELEASE.  Payload goes by reference into the assembler's arena.  `releasable` says how many of the oldest
 *  reported-and-unreleased messages no queue entry refers to after this call, in the unit grdma_h2_asm_release counts
 *  in (every reported descriptor is one, NO_SPACE ones too): messages finished in this call, dropped by status,
 *  unrouted, dropped as closed, of a lost call.  A source call that is new but was not taken is not covered.  Release
 *  them behind the send that gathers this call's slices.
 * RESULT BLOCK out[16]: {0 finished, 1 still pending, 2 slices, 3 header-arena bytes, 4 wire bytes, 5 flow-controlled
 *  bytes granted, 6 stall bits (1 = the connection's window, 2 = a stream's), 7 overflow, 8 taken new (descriptors
 *  appended to the queue), 9 dropped by status, 10 unrouted, 11 dropped closed, 12 releasable, 13 flags (GRDMA_H2_WR_LOST),
 *  14 framing time in us (HIP events, the four launches), 15 spare: 0}.  Returns the slice count.
 * MIXING.  grdma_h2_sw_frame and grdma_h2_sw_intake on the same sw between windowed replies are allowed and consistent:
 *  the windows are one state, and the queue owns its progress words.
 * -GRDMA_ERR_INVALID (grdma_last_error says why): no attachment, send windows or parser gone, null, zero or misaligned
 *  (16 bytes) targets, unknown flags.
 * Not here: the windowed reply inside a pipe or group pipe (a job's graph carries a fixed slice count per step). */
enum { GRDMA_H2_WR_PENDING_ONLY = 1 };  /* flags of a call */
enum { GRDMA_H2_WR_LOST = 1 };          /* flags word of the result block */
int grdma_h2_reply_attach_windows(grdma_h2_reply* reply, grdma_h2_sw* sw, uint32_t max_pending);
int64_t grdma_h2_reply_frame_windowed(grdma_h2_reply* reply, uint32_t flags, grdma_slice* d_slices_out, uint64_t slices_cap,
                                      void* d_hdr_arena, uint64_t hdr_cap, uint64_t out[16]);
/* the queue as it is, unfinished entries in order: per entry {outgoing stream, message length, flow-controlled bytes
 * sent} in out[3 i .. 3 i + 2], at most cap entries written; returns their number */
int64_t grdma_h2_reply_pending(grdma_h2_reply* reply, uint64_t* out, uint64_t cap);
/* grdma_h2_reply_frame_windowed for n replies (1 .. GRDMA_H2_BATCH_MAX) in the same four launches (k_h2_links_wr_queue,
 * k_h2_links_sw_plan, k_h2_links_sw_emit, k_h2_links_wr_commit): every item frames its own queue and source call under
 * its own windows into its own targets, exactly as the single call does.  An item's overflow (1 or 2) and its LOST flag
 * stay with the item: n_slices is -GRDMA_ERR_CAPACITY there and the other items are exact.  Returns the number of items
 * without overflow, or a negative error.  -GRDMA_ERR_INVALID (nothing runs, nothing changes): n outside the range, a NULL
 * array, an item without reply, the same reply, source assembler or send windows twice, and per item what the single
 * call refuses. */
typedef struct grdma_h2_wr_item {
  grdma_h2_reply* reply;      /* distinct, attached to distinct send windows, of distinct source assemblers */
  uint32_t flags;             /* GRDMA_H2_WR_PENDING_ONLY */
  uint32_t pad;
  grdma_slice* d_slices_out;  /* device slice table of the item */
  uint64_t slices_cap;
  void* d_hdr_arena;          /* device header arena of the item, 32 bytes per frame */
  uint64_t hdr_cap;
  int64_t n_slices;           /* out: the single call's return value */
  uint64_t out[16];           /* out: the single call's result block; out[14] is the batch's time, repeated */
} grdma_h2_wr_item;
int grdma_h2_reply_frame_windowed_batch(grdma_h2_wr_item* items, uint32_t n);

/* ---- Control replies on the device: SETTINGS ACK, PING ACK, RST_STREAM (csrc/grdma_h2_ctl.h) ----
 * The frames HTTP/2 obliges a transport to answer, written in device memory from a deframing's events, so that a
 * connection stays alive with no host step between the deframer and the wire.  One control-reply writer per parser,
 * independent of the ledger (grdma_h2_fc) and the send windows (grdma_h2_sw): all three may consume the same deframing
 * in any order, each keeps its own count of the calls it has taken.  The sequential reference is
 * tests/h2_control_model.py.
 * 1. INPUT.  grdma_h2_ctl_reply takes in the LAST standalone deframing of the parser (grdma_h2_deframe or
 *    grdma_h2_deframe_messages): its device event list, its slice table and its receive arena, which must still hold the
 *    call's bytes; it is ordered behind that deframing on the device.  A frame's payload is the run of PAYLOAD events
 *    behind its FRAME event; PAYLOAD events in front of the call's first FRAME event continue the frame the previous
 *    call's end cut (the carry).  Every frame ends with a PAYLOAD event whose is_last is 1: the frame's completion.
 * 2. REPLIES DUE.  SETTINGS without ACK: one SETTINGS ACK (00 00 00 04 01 00 00 00 00), in the call that completes the
 *    frame.  PING without ACK: one PING ACK (00 00 08 06 01 00 00 00 00 + the 8 opaque bytes, read from the arena), in
 *    the call that completes it.  A stream error -- a FRAME event whose status byte (b >> 8) is not 0, or a FRAME event
 *    of type 0xff (stream in c) -- one RST_STREAM(stream, PROTOCOL_ERROR = 1) (00 00 04 03 00 + stream id + 00 00 00
 *    01), in the call that holds the event.  The deframer reports each at most once; the writer does not deduplicate.
 *    EVERY PING is answered: there is no ping-abuse policy, max_replies is the flood bound.
 * 3. ORDER.  The PING ACKs first, in the order of their completions, then the SETTINGS ACKs and RST_STREAMs in the
 *    order of their events.  RFC 7540 fixes no order between them: this is a fixed choice (the reference transport
 *    flushes its ping acks in front of its queued control frames when it begins a write).
 * 4. OUTPUT, in the ledger's form: the concatenated frames in a header arena, 32 bytes of arena per slice, cut into
 *    23-byte inlined slices (the last one shorter), as grpc_slice_buffer_add makes of small inlined slices; the 9 bytes
 *    behind a slice's 23 are not written.  The list is an outbuf of its own.  Result block: {frames, slices, wire bytes,
 *    SETTINGS ACKs, PING ACKs, RST_STREAMs, flags (grdma_h2_ctl_flag), overflow}.  Returns the slice count.
 * 5. WHAT THE PEER SAID (grdma_h2_ctl_peer): {SETTINGS ACKs received, PING ACKs received, the 8 opaque bytes of the last
 *    PING ACK as a little-endian word of the wire bytes, GOAWAY frames received, last_stream_id of the last GOAWAY (bit
 *    31 cleared), its error code, the number of the call (grdma_h2_ctl_stats word 0 behind it) that completed it, 0}.
 *    "Last" is by completion within a call, by call order across calls.  GOAWAY debug data is skipped.
 * 6. THE CARRY.  A call's end may cut one frame: its type and flags and, of a PING or GOAWAY, those of its first 8
 *    payload bytes that are in.  Its reply or its record is due in the call that completes it.
 * 7. ERRORS AND CAPS.  A call that ended with a connection error writes and records nothing, is taken, the carry goes.
 *    A call whose event list overflowed sets the sticky flag GRDMA_H2_CTL_LOST, returns -GRDMA_ERR_CAPACITY with
 *    overflow word 2, is taken, the carry goes, the record keeps what it knows.  A standalone deframing that was never
 *    taken in (the send windows' "skipped" rule) sets the flag and drops the carry; the call itself is answered.  More
 *    replies than max_replies, or a slice or header cap too small: overflow word 1, -GRDMA_ERR_CAPACITY, the result
 *    block holds the totals, NOTHING is written and NOTHING is committed -- carry and record stay, the call is NOT taken
 *    and may be repeated with larger targets while the deframing's buffers stand (unlike the ledger, whose bytes were
 *    counted already: an unanswered PING must not be lost).
 * -GRDMA_ERR_INVALID or NULL (grdma_last_error says why; nothing runs, nothing changes): a second writer on a parser,
 * max_replies outside 1 .. 2^24, no call yet or a call taken in already, a parser that is gone (destroy still works),
 * null, zero or misaligned (16 bytes) targets; in the batch n outside 1 .. GRDMA_H2_BATCH_MAX, a NULL item, the same
 * writer twice.
 * Not here: replies to a pipe's or group pipe's steps, the other settings (HPACK: grdma_h2_hpack and grdma_h2_hpenc
 * below). */
enum grdma_h2_ctl_flag { GRDMA_H2_CTL_LOST = 1, GRDMA_H2_CTL_GOAWAY = 2 /* a GOAWAY completed in this call */ };
typedef struct grdma_h2_ctl grdma_h2_ctl;
grdma_h2_ctl* grdma_h2_ctl_create(grdma_h2_parser* parser, uint32_t max_replies);  /* 1 .. 2^24; one per parser */
void grdma_h2_ctl_destroy(grdma_h2_ctl* ctl);
int64_t grdma_h2_ctl_reply(grdma_h2_ctl* ctl, grdma_slice* d_slices_out, uint64_t slices_cap, void* d_hdr_arena, uint64_t hdr_cap,
                           uint64_t out[8]);
int grdma_h2_ctl_peer(grdma_h2_ctl* ctl, uint64_t out[8]);
/* {calls taken, SETTINGS ACKs written, PING ACKs written, RST_STREAMs written, wire bytes written, 0, the LOST flag,
 * kernel time of the last call in NANOseconds (HIP events)} */
int grdma_h2_ctl_stats(grdma_h2_ctl* ctl, uint64_t out[8]);
/* grdma_h2_ctl_reply for n writers (1 .. GRDMA_H2_BATCH_MAX) in the same four launches (k_h2_links_ctl_*): every item
 * answers the last standalone deframing of its OWN parser into its own targets, exactly as the single call does.  out: 8
 * result words per item, in item order.  An item's overflow (word 1: not taken, may be repeated; word 2: lost) stays with
 * the item, the other items are exact; the return value is the number of items without overflow, or a negative error. */
typedef struct grdma_h2_ctl_item {
  grdma_h2_ctl* ctl;          /* distinct */
  grdma_slice* d_slices_out;  /* device slice table of the item */
  uint64_t slices_cap;
  void* d_hdr_arena;          /* device header arena of the item, 32 bytes per slice */
  uint64_t hdr_cap;
} grdma_h2_ctl_item;
int grdma_h2_ctl_reply_batch(const grdma_h2_ctl_item* items, uint32_t n, uint64_t* out);

/* ---- Header blocks: HPACK on the device (csrc/grdma_h2_hpack.h) ----
 * The header blocks of a deframing's HEADERS and CONTINUATION frames, decoded (RFC 7541) into device memory: a block
 * table, a field table and a string arena.  One header decoder per parser, a sibling of the control-reply writer:
 * independent of the ledger, the send windows and the writer -- any of them may consume the same deframing in any order
 * -- with its own count of the calls it has taken.  The sequential reference is tests/h2_hpack_model.py.
 * 1. BLOCK.  grdma_h2_hpack_decode takes in the LAST standalone deframing of the parser (events, slice table, receive
 *    arena, which must still hold the call's bytes) and is ordered behind it on the device.  A block is the payload of
 *    a HEADERS frame and of the CONTINUATION frames behind it up to the frame with END_HEADERS (0x4); the HEADERS
 *    payload loses the pad-length byte (PADDED, 0x8), then 5 priority bytes (PRIORITY, 0x20), and the padding at its
 *    end.  ERR_PADDING: a padded or prioritised frame shorter than those bytes, a pad length >= what is left.  A block
 *    is decoded in the call that completes its last frame.  PUSH_PROMISE is no block.  A block on a stream the deframer
 *    refused is decoded and delivered like any other (the table must stay in step); the status byte of its FRAME event
 *    rides in the block's flags.
 * 2. CARRY.  A block the call's end cuts keeps its fragment bytes in the decoder's device buffer (max_block_bytes), the
 *    open frame's type, flags and size, the payload bytes seen and the pad length if it is in; PAYLOAD events in front
 *    of the call's first FRAME event continue it.  A block above max_block_bytes: ERR_BLOCK_TOO_LARGE.
 * 3. HPACK.  Integers need not be minimal; more than five continuation bytes or a value above 2^32 - 1: ERR_INTEGER.
 *    Huffman padding is at most 7 one-bits and EOS inside a string is an error: ERR_HUFFMAN; a length or an integer that
 *    runs past the block: ERR_TRUNCATED.  Index 0 or one beyond the live table: ERR_INDEX (1..61 static, 62 the newest
 *    dynamic entry).  A size update stands in front of the block's first field, may come more than once and is <= our
 *    setting, else ERR_SIZE_UPDATE; a lowered setting takes effect at once and need not be acknowledged by one.  Entry
 *    size 32 + name + value; an insertion evicts from the oldest until the entry fits; an entry larger than the table
 *    empties it and is not inserted; a name reference to an entry the same insertion evicts is valid (4.4).  A block
 *    with several faults reports the first in wire order among integers, lengths, Huffman strings and size updates, and
 *    ERR_INDEX only where there is none of those.
 * 4. OUTPUT.  Blocks in completion order, a block's fields contiguous in wire order, the string arena byte-contiguous:
 *    name then value, field after field, no terminators; indexed fields copy their bytes too.  Nothing is written
 *    behind the three totals.  Result block: {blocks, fields, string bytes, entries inserted, entries evicted, table
 *    bytes after the call, flags (grdma_h2_hpack_flag) | error << 8 | failing stream << 32, overflow}.
 * 5. ERRORS.  An error in block k of a call delivers and commits blocks 0..k-1 and sets FAILED with the error and the
 *    stream; it is sticky: every later call is taken, writes nothing and returns 0 with the word.  The same end state,
 *    with its own flag or code: a call that ended with a connection error of the deframer (FAILED, ERR_DEFRAMER), an
 *    overflowed event list (LOST, -GRDMA_ERR_CAPACITY, overflow word 2), a deframing never taken in (LOST).
 * 6. CAPS.  More blocks, fields or string bytes than the caps: overflow word 1, -GRDMA_ERR_CAPACITY, the result block
 *    holds the totals, NOTHING is written and NOTHING is committed (table, carry, counters), the call is NOT taken and
 *    may be repeated with larger targets while the deframing's buffers stand.
 * -GRDMA_ERR_INVALID or NULL (grdma_last_error says why; nothing runs, nothing changes): a second decoder on a parser,
 * max_table_size above 65536, max_block_bytes outside 64 .. 2^20, no call yet or a call taken in already, a parser that
 * is gone (destroy still works), null, zero or misaligned (16 bytes) targets; in the batch n outside 1 ..
 * GRDMA_H2_BATCH_MAX, a NULL item array, result array or decoder, the same decoder twice.
 * MANY LINKS.  grdma_h2_hpack_decode_batch is grdma_h2_hpack_decode for n decoders (1 .. GRDMA_H2_BATCH_MAX) in six
 * launches however many (k_h2_links_hpack_*): the gather of every link, one host step that sizes each decoder's own
 * scratch by its own figure, the five other stages of every link.  Every item decodes the last standalone deframing of
 * its OWN parser into its own targets against its own table, by rules 1 to 6 exactly as the single call does; the call
 * is ordered behind every listed parser.  out: 8 result words per item, in item order.  A sticky error, a lost call, a
 * deframer error or an overflow (word 1: not taken, may be repeated alone or in a later batch; word 2: lost) stay with
 * the item, the other items are exact; the return value is the number of items whose overflow word is 0, or a negative
 * error.  An item whose deframing holds more than 2^30 header bytes refuses the whole call (-GRDMA_ERR_INVALID) behind
 * the gather, which commits nothing: nothing is taken.  set_max_table_size stays per decoder.
 * Not here: the decoder inside a pipe, SETTINGS_MAX_HEADER_LIST_SIZE, PUSH_PROMISE.  (The HPACK encoder: "Header
 * blocks, sending" below; gRPC's metadata validation: "Call metadata" behind it.) */
enum grdma_h2_hpack_flag { GRDMA_H2_HPACK_FAILED = 1, GRDMA_H2_HPACK_LOST = 2, GRDMA_H2_HPACK_OPEN = 4 /* a block is cut by the call's end */ };
enum grdma_h2_hpack_error {
  GRDMA_H2_HPACK_ERR_PADDING = 1, GRDMA_H2_HPACK_ERR_BLOCK_TOO_LARGE = 2, GRDMA_H2_HPACK_ERR_INTEGER = 3, GRDMA_H2_HPACK_ERR_TRUNCATED = 4,
  GRDMA_H2_HPACK_ERR_HUFFMAN = 5, GRDMA_H2_HPACK_ERR_INDEX = 6, GRDMA_H2_HPACK_ERR_SIZE_UPDATE = 7, GRDMA_H2_HPACK_ERR_DEFRAMER = 8
};
typedef struct grdma_h2_header_field { uint32_t name_off, value_off, name_len, value_len; } grdma_h2_header_field;
    /* offsets into the string arena; name_len bits 24..31: representation 0 indexed, 1 incremental, 2 without, 3 never indexed */
typedef struct grdma_h2_header_block { uint32_t stream, first_field, nfields, flags; } grdma_h2_header_block;
    /* flags: 1 END_STREAM of the HEADERS frame, 2 it carried PRIORITY, bits 8..15 the status byte of its FRAME event */
typedef struct grdma_h2_hpack grdma_h2_hpack;
grdma_h2_hpack* grdma_h2_hpack_create(grdma_h2_parser* parser, uint32_t max_table_size /* our SETTINGS_HEADER_TABLE_SIZE, 0 .. 65536 */,
                                      uint32_t max_block_bytes /* 64 .. 2^20 */);
void grdma_h2_hpack_destroy(grdma_h2_hpack* hpack);
int grdma_h2_hpack_set_max_table_size(grdma_h2_hpack* hpack, uint32_t max_table_size);  /* the bound for the peer's later size updates */
int64_t grdma_h2_hpack_decode(grdma_h2_hpack* hpack, grdma_h2_header_block* d_blocks, uint64_t blocks_cap,
                              grdma_h2_header_field* d_fields, uint64_t fields_cap, void* d_strings, uint64_t strings_cap,
                              uint64_t out[8]);  /* returns the block count */
/* the live dynamic table, newest first, into host memory: per entry two 32-bit lengths (name, value), then the name's and
 * the value's bytes.  out: {entries, bytes of the dump, table bytes (RFC 7541 4.1), the size limit in force}; a buffer too
 * small (NULL with cap 0 asks for the figures): -GRDMA_ERR_CAPACITY with out filled in */
int grdma_h2_hpack_table(grdma_h2_hpack* hpack, void* host_buf, uint64_t cap, uint64_t out[4]);
/* {calls taken, blocks, fields, string bytes, inserts, evictions, the sticky flags word, kernel time of the last call in
 * NANOseconds (HIP events)} */
int grdma_h2_hpack_stats(grdma_h2_hpack* hpack, uint64_t out[8]);
typedef struct grdma_h2_hpack_item {
  grdma_h2_hpack* hpack;            /* distinct */
  grdma_h2_header_block* d_blocks;  /* the item's device targets, as grdma_h2_hpack_decode's */
  uint64_t blocks_cap;
  grdma_h2_header_field* d_fields;
  uint64_t fields_cap;
  void* d_strings;
  uint64_t strings_cap;
} grdma_h2_hpack_item;
int grdma_h2_hpack_decode_batch(const grdma_h2_hpack_item* items, uint32_t n_items, uint64_t* out /* 8 words per item */);

/* ---- Header blocks, sending: the HPACK encoder on the device (csrc/grdma_h2_hpenc.h) ----
 * Header lists in device memory encoded (RFC 7541) into the wire bytes of HEADERS and CONTINUATION frames: the response
 * headers and the trailers around a reply's DATA, or a proxy's re-encoding of what it has just decoded against the next
 * hop's dynamic table.  One header encoder per connection, resident in device memory; it belongs to no parser (it is the
 * sending side).  The call is ordered on the stream of the standalone HTTP/2 calls: a grdma_h2_hpack_decode immediately
 * in front of it needs no host synchronisation.  The sequential reference, which defines the exact bytes, is
 * tests/h2_hpenc_model.py.
 * 1. INPUT, all in device memory: nblocks grdma_h2_header_block, nfields grdma_h2_header_field and a string arena of
 *    strings_bytes bytes -- exactly the decoder's OUTPUT layout.  Of a block: stream, first_field / nfields (blocks may
 *    share fields), flags bit 0 END_STREAM, its other bits are ignored.  Of a field: name_len bits 24..31 are the
 *    caller's HINT, of which the low two bits are read: 0 or 1 (indexable) -- indexed if a full match is live, else a
 *    literal WITH incremental indexing, which is inserted; 2 -- indexed if a full match is live, else a literal without
 *    indexing; 3 -- always a literal never-indexed, even when a full match is live (a sensitive value must not turn into
 *    an index).  Decoder output therefore forwards unchanged.
 * 2. MATCHING runs against the table as it stands in front of the field: the static table and the dynamic entries live
 *    at that moment, those inserted by earlier fields of this call included.  Full match (name and value equal): the
 *    lowest static index if there is one, else the NEWEST dynamic entry.  Name reference of a literal: the lowest static
 *    index whose name is equal, else the newest dynamic entry whose name is equal, else index 0 with a literal name; it
 *    is resolved in front of the evictions of the field's own insertion (RFC 7541 4.4).  Equality is of bytes; the hash
 *    (FNV-1a) finds candidates and never decides.
 * 3. STRINGS AND INTEGERS.  A string is Huffman-coded where that is NOT LONGER than its raw bytes -- names and values
 *    alike; RFC 7541 Appendix C.6.2 codes "307" in three bytes -- and the empty string goes raw; padding is one-bits;
 *    integers are minimal.
 * 4. TABLE.  RFC 7541 4: entry size 32 + name + value; an insertion evicts from the oldest until the entry fits; an
 *    entry larger than the table empties it, is not inserted and is still sent as a literal with incremental indexing
 *    (the peer's table empties too).  The limit is the peer's SETTINGS_HEADER_TABLE_SIZE, at most 65536 bytes and 2048
 *    live entries as the decoder has it.  Both sides begin at 4096, or at peer_table_size where that is less (no size
 *    update is sent for it: Appendix C.6); grdma_h2_hpenc_set_peer changes the limit between calls, on the host alone:
 *    the next call that sends a block opens its FIRST block with one size update when the size differs from what the
 *    peer's decoder is at -- a create above 4096 counts -- or with two, the smallest since the last block and then the
 *    final one, when it was lowered and then raised (4.2).  The evictions happen first, in front of the block's fields.
 * 5. FRAMES.  Per block one HEADERS frame -- 9-byte header, END_STREAM from the block's flags, no padding, no priority
 *    -- then CONTINUATION frames, each full frame of the peer's max frame size; END_HEADERS on the last.  An empty block
 *    is a HEADERS frame without payload.  Blocks are contiguous in the wire arena, in input order; the block-wire table
 *    says per block where its frames begin, how many bytes they are and how many frames, so that the caller can put them
 *    in front of or behind its DATA slices.  Result block: {blocks, frames, wire bytes, entries inserted, entries
 *    evicted, table bytes after the call, flags (grdma_h2_hpenc_flag) | error << 8 | offending block << 32, overflow}.
 * 6. CAPS.  A wire arena or a block-wire table too small: overflow word 1, -GRDMA_ERR_CAPACITY, the result block holds
 *    the totals, NOTHING is written and NOTHING is committed (table, counters, pending size updates); the same call
 *    with larger targets gives exactly what a never-refused call gives.
 * 7. BAD INPUT is found on the device, where the input lives: a block whose field range leaves the field table
 *    (ERR_FIELD_RANGE), a stream id of 0 or above 2^31 - 1 (ERR_STREAM), a value length above 2^24 - 1 (ERR_LENGTH), a
 *    string that leaves the arena (ERR_STRING) -- the first block with a fault; in it the range, then the stream, then
 *    its first faulty field, the length first -- and a block whose frames pass 2^32 - 1 bytes (ERR_BLOCK_TOO_LARGE).
 *    The flag is BAD_INPUT with the code and the block's number, the other result words are 0 but the table bytes;
 *    nothing is written, nothing is committed, the call returns -GRDMA_ERR_INVALID.  Not sticky: the encoder's state is
 *    untouched.
 * -GRDMA_ERR_INVALID or NULL (grdma_last_error says why; nothing runs, nothing changes): null, zero or misaligned (16
 * bytes) wire arena or block-wire table, a null input table with a count above 0, a misaligned block or field table, a
 * table size above 65536, a max frame size outside 16384 .. 2^24 - 1, 2^32 - 1 blocks or more; in the batch n outside
 * 1 .. GRDMA_H2_BATCH_MAX, a NULL item array, result array or encoder, the same encoder twice, any item the single
 * call's argument checks refuse.
 * MANY LINKS.  grdma_h2_hpenc_encode_batch is grdma_h2_hpenc_encode for n encoders (1 .. GRDMA_H2_BATCH_MAX) in four
 * launches however many (k_h2_links_hpenc_*), ordered on the same stream: a grdma_h2_hpack_decode_batch immediately in
 * front of it needs no host synchronisation.  Every item encodes its own input into its own wire arena and block-wire
 * table against its own peer table, with its own pending size updates and its own max frame size, by rules 1 to 7
 * exactly as the single call does.  Input tables may be shared between items (a proxy fans one header list out to
 * many links); overlapping wire arenas are the caller's error and are not checked.  out: 8 result words per item, in
 * item order.  Bad input (the BAD_INPUT flag, the code and the block in the item's words) and a cap overflow (overflow
 * word 1: nothing of the item is written or committed, its size updates stay pending, it may be repeated alone or in a
 * later batch and then gives what a never-refused call gives) stay with the item, the other items are exact.  The
 * return value is the number of items whose blocks are on the wire (overflow word 0 and no BAD_INPUT; an item without
 * blocks counts, and commits no peer settings), or a negative error.  The call's words go up and the result words come
 * down in ONE copy each, whatever n.  Items whose blocks share fields so that their occurrences pass nfields + 64 get
 * their occurrence table grown and run once more, in a second run of the four launches over those items only; an item
 * that then still asks for more, or that holds 2^32 - 1 occurrences or more, refuses the call (-GRDMA_ERR_INVALID):
 * that item and the ones waiting with it are untouched, but THE ITEMS THAT STOOD IN THE FIRST RUN STAY COMMITTED --
 * their bytes are on the wire, their tables and counters moved, and their result words are in out.
 * grdma_h2_hpenc_stats word 7 and grdma_h2_hpenc_last_stages report the batch's sections, repeated for every item.
 * Not here: the encoder as a stage of a reply pipe or of the group pipe, gRPC's per-key metadata policy (which keys
 * are indexable is the caller's hint). */
enum grdma_h2_hpenc_flag { GRDMA_H2_HPENC_BAD_INPUT = 1 };
enum grdma_h2_hpenc_error {
  GRDMA_H2_HPENC_ERR_FIELD_RANGE = 1, GRDMA_H2_HPENC_ERR_STREAM = 2, GRDMA_H2_HPENC_ERR_LENGTH = 3, GRDMA_H2_HPENC_ERR_STRING = 4,
  GRDMA_H2_HPENC_ERR_BLOCK_TOO_LARGE = 5
};
typedef struct grdma_h2_hpenc grdma_h2_hpenc;
typedef struct grdma_h2_header_wire { uint64_t off; uint32_t len, nframes; } grdma_h2_header_wire;
    /* a block's frames: offset in the wire arena, bytes (frame headers included), frames */
grdma_h2_hpenc* grdma_h2_hpenc_create(uint32_t peer_table_size /* 0 .. 65536 */, uint32_t peer_max_frame /* 16384 .. 2^24 - 1 */);
void grdma_h2_hpenc_destroy(grdma_h2_hpenc* enc);
int grdma_h2_hpenc_set_peer(grdma_h2_hpenc* enc, uint32_t peer_table_size, uint32_t peer_max_frame);
int64_t grdma_h2_hpenc_encode(grdma_h2_hpenc* enc, const grdma_h2_header_block* d_blocks, uint64_t nblocks,
                              const grdma_h2_header_field* d_fields, uint64_t nfields, const void* d_strings, uint64_t strings_bytes,
                              void* d_wire, uint64_t wire_cap, grdma_h2_header_wire* d_block_wire, uint64_t block_wire_cap,
                              uint64_t out[8]);  /* returns the frame count */
/* the encoder's view of the peer's dynamic table, in the dump format of grdma_h2_hpack_table */
int grdma_h2_hpenc_table(grdma_h2_hpenc* enc, void* host_buf, uint64_t cap, uint64_t out[4]);
/* {calls, blocks, fields, header-list bytes in, wire bytes out, inserts, evictions, kernel time of the last call in
 * NANOseconds (HIP events)} */
int grdma_h2_hpenc_stats(grdma_h2_hpenc* enc, uint64_t out[8]);
/* the last call's kernel time by stage, NANOseconds: {scan, walk, emit and commit, total} */
int grdma_h2_hpenc_last_stages(grdma_h2_hpenc* enc, uint64_t out[4]);
typedef struct grdma_h2_hpenc_item {
  grdma_h2_hpenc* enc;                    /* distinct */
  const grdma_h2_header_block* d_blocks;  /* the item's device input and targets, as grdma_h2_hpenc_encode's */
  uint64_t nblocks;
  const grdma_h2_header_field* d_fields;
  uint64_t nfields;
  const void* d_strings;
  uint64_t strings_bytes;
  void* d_wire;
  uint64_t wire_cap;
  grdma_h2_header_wire* d_block_wire;
  uint64_t block_wire_cap;
} grdma_h2_hpenc_item;
int grdma_h2_hpenc_encode_batch(const grdma_h2_hpenc_item* items, uint32_t n_items, uint64_t* out /* 8 words per item */);

/* ---- Call metadata: gRPC's reading of decoded header blocks on the device (csrc/grdma_h2_meta.h) ----
 * The tables the header decoder writes, read where they lie: one fixed-size CALL RECORD per header block -- its kind, a
 * verdict, the method id from a path list registered at creation, the timeout, the encoding, the HTTP and the gRPC
 * status, the field indices of the strings a later stage wants -- and a compact REJECTION LIST, one
 * grdma_h2_header_block per request the server must refuse, each pointing into a constant field table and string arena
 * the reader owns in device memory, so that grdma_h2_hpenc_encode turns the list into Trailers-Only responses with no
 * host step and no per-call string work.  The reader is stateless between calls apart from its counters and belongs to
 * no parser.  The call is ordered on the stream of the standalone HTTP/2 calls: a grdma_h2_hpack_decode in front of it
 * and a grdma_h2_hpenc_encode behind it need no host synchronisation (the host knows the three counts from the
 * decoder's result block).  The sequential reference, which defines the exact output, is tests/h2_meta_model.py.
 * CREATE.  methods is host memory: nmethods entries back to back, each a 32-bit little-endian length and the path's
 * bytes (the dump style of grdma_h2_hpack_table); a method's id is its position.  nmethods 0 .. 4096, a path 1 .. 1024
 * bytes.  accept_encodings: bit 0 identity, bit 1 gzip, bit 2 deflate.  NULL (grdma_last_error says why) for a path
 * twice, a list that does not end at exactly methods_bytes, accept_encodings with bits above 7 or without bit 0.  On
 * the device the paths live in an open-addressed table of a power of two >= 2 nmethods slots (FNV-1a, linear probing);
 * the hash finds candidates and bytes decide.
 * 1. INPUT, all in device memory, by the encoder's input rules: blocks may share fields; of a block only stream,
 *    first_field, nfields and flags bit 0 (END_STREAM) are read; bits 24..31 of name_len are ignored.  BAD INPUT is
 *    found on the device: a block whose field range leaves the field table (ERR_FIELD_RANGE), a stream id of 0 or above
 *    2^31 - 1 (ERR_STREAM), a string that leaves the arena (ERR_STRING) -- the first block with a fault; in it the
 *    range, then the stream, then the strings.  Result word 6 is BAD_INPUT | code << 8 | block << 32, the other words
 *    are 0, nothing is written, no counter moves, the call returns -GRDMA_ERR_INVALID.  Not sticky.
 * 2. FIELDS.  Known keys: :method :scheme :path :authority :status, content-type te grpc-timeout grpc-encoding
 *    grpc-accept-encoding grpc-status grpc-message, and the connection-specific names connection keep-alive
 *    proxy-connection transfer-encoding upgrade.  A field is BAD when its name is empty; when its name has a byte
 *    outside a-z 0-9 - _ . (upper case included; a ':' at position 0 is allowed); when it starts with ':' and is none
 *    of the five pseudo-headers; when its name does not end in -bin and its value has a byte outside 0x20 .. 0x7e; when
 *    its name is connection-specific; when it is te with a value other than trailers.
 * 3. KIND, from content alone (no per-stream state): a block with any of the four request pseudo-headers is a REQUEST;
 *    else a block with :status is a RESPONSE; else it is TRAILERS (the empty block too).
 * 4. A block is MALFORMED (the stream error PROTOCOL_ERROR of RFC 7540 8.1.2.6) when it holds a bad field; has a
 *    pseudo-header (a name that starts with ':') behind a regular field; has a pseudo-header twice; has :status
 *    together with a request pseudo-header; is a REQUEST without :method, :scheme or :path, with a :scheme other than
 *    http or https or with an empty :path; is a RESPONSE whose first :status is not exactly three digits.  bad_field
 *    names the first offending field in block order: the bad field, the pseudo-header that came late, the second
 *    occurrence, the later of :status and the request pseudo-header beside it, the :scheme or the empty :path, the
 *    :status; a missing pseudo-header offends nowhere (none).
 * 5. Known keys: the FIRST occurrence wins (a bad field's too); later ones count in nothing.
 * 6. VALUES.  grpc-timeout: 1 to 8 digits and one of H M S m u n, in nanoseconds, saturated at 2^63 - 1 (2562047H is
 *    exact, 2562048H saturates; compared before it is multiplied); anything else is BAD_TIMEOUT.  content-type is good
 *    when it is application/grpc, alone or followed by '+' or ';' and anything.  grpc-encoding: identity 0, gzip 1,
 *    deflate 2, any other value 255; 0 without the key.  grpc-status: 1 to 3 digits.  :method is good when it is POST.
 *    The method id is the lookup of :path.  path_field, authority_field and message_field name the first occurrence,
 *    as an index into the FIELD TABLE.  http_status is the number of a three-digit :status, grpc_status that of a
 *    good grpc-status, else none.  ncustom counts the fields whose name is none of the known keys.
 * 7. VERDICT, the first that applies: MALFORMED (rule 4); BAD_METHOD (REQUEST, :method not POST); BAD_CONTENT_TYPE
 *    (REQUEST or RESPONSE; missing counts as bad); BAD_TE (REQUEST without te: trailers); BAD_TIMEOUT (rule 6);
 *    UNIMPLEMENTED (REQUEST, path not registered); BAD_ENCODING (REQUEST, encoding 255 or not in accept_encodings);
 *    HTTP_STATUS (RESPONSE, :status other than 200); NO_STATUS (a RESPONSE or TRAILERS with END_STREAM and without
 *    grpc-status); BAD_GRPC_STATUS (grpc-status present and not 1 to 3 digits); else OK.  Flags: HAS_TIMEOUT (a good
 *    one), END_STREAM, HAS_GRPC_STATUS and HAS_MESSAGE (the key is present).
 * 8. REJECTIONS.  Every REQUEST whose verdict is neither OK nor MALFORMED gets one block in d_reject, in input order,
 *    compacted: {the request's stream, first_field / nfields into the reader's constant tables
 *    (grdma_h2_meta_reject_tables), flags 1}.  The constant lists, every field with hint 1, are a FIXED POLICY, as flow
 *    control is -- :status / grpc-status: BAD_METHOD 405 / 13, BAD_CONTENT_TYPE 415 / 13, BAD_TE 400 / 13, BAD_TIMEOUT
 *    400 / 13, UNIMPLEMENTED 200 / 12, BAD_ENCODING 200 / 12 -- with content-type: application/grpc between the two and
 *    a fixed grpc-message behind them (csrc/grdma_h2_meta_tables.h spells it); BAD_ENCODING adds grpc-accept-encoding
 *    with the create-time set.  A MALFORMED request gets no block: its RST_STREAM is the control-reply writer's side
 *    and is not here.
 * 9. RESULT BLOCK: {blocks, requests, responses, trailers, rejections, malformed, flags (grdma_h2_meta_flag) | error <<
 *    8 | offending block << 32, overflow}.
 * 10. CAPS.  meta_cap < nblocks or reject_cap < rejections: overflow word 1, -GRDMA_ERR_CAPACITY, the result block
 *    holds the totals, NOTHING is written to either target and no counter moves; the same call with larger targets
 *    gives what a never-refused call gives.  Nothing is written behind the totals in any case.
 * 11. -GRDMA_ERR_INVALID (grdma_last_error says why; nothing runs, nothing changes): null, zero-cap or misaligned (16
 *    bytes) targets, a null input table with a count above 0, a misaligned block or field table, 2^32 - 1 blocks or
 *    more, no reader, no result array; in the batch n outside 1 .. GRDMA_H2_BATCH_MAX, a NULL item array or result
 *    array, any item the single call's argument checks refuse -- out is not touched.
 * MANY LINKS.  grdma_h2_meta_read_batch is grdma_h2_meta_read for n items (1 .. GRDMA_H2_BATCH_MAX) in three launches
 * however many (k_h2_links_meta_*), ordered on the same stream: a grdma_h2_hpack_decode_batch in front of it and a
 * grdma_h2_hpenc_encode_batch behind it need no host synchronisation.  ONE reader, n items, by design (unlike the
 * encoder, whose state is per connection): the method table, the accepted encodings and the constant rejection tables
 * belong to the server and are the same on every link, so an item is one link's decoder output and that link's two
 * targets.  Every item is read by rules 1 to 10 exactly as the single call reads it: its record table, its rejection
 * list and its eight result words are byte for byte what grdma_h2_meta_read gives for the same arguments.  Input tables
 * may be shared between items; overlapping targets are the caller's error and are not checked.  The rejection blocks of
 * every item point into the reader's one pair of constant tables (grdma_h2_meta_reject_tables): an encode batch passes
 * that pair as the field table and string arena of every item.  out: 8 result words per item, in item order.  Bad input
 * (the BAD_INPUT flag, the code and the block in the item's word 6, its other words 0) and a cap overflow (overflow
 * word 1 and the totals, nothing written to either of its targets; repeated alone or in a later batch it gives what a
 * never-refused call gives) stay with the item, the other items are exact.  The return value is the number of items
 * read (overflow word 0 and no BAD_INPUT; an item with 0 blocks counts), or a negative error.  COUNTERS: the call is
 * ONE call in grdma_h2_meta_stats, which moves by the sums of blocks, requests, responses, trailers, rejections and
 * malformed over the items that were read and by nothing for the others; a batch in which no item was read moves no
 * counter, as a refused single call moves none.  Word 7 is the batch's kernel time.  All items' call words go up in
 * ONE copy and all result words come down in ONE copy, whatever n.
 * Not here: the reader inside a pipe or a group pipe, a grid per link sized by the link's block count,
 * percent-decoding of grpc-message (the record names the field), base64 of -bin values, SETTINGS_MAX_HEADER_LIST_SIZE, RST_STREAM for malformed blocks. */
enum grdma_h2_meta_flag { GRDMA_H2_META_BAD_INPUT = 1 };
enum grdma_h2_meta_error { GRDMA_H2_META_ERR_FIELD_RANGE = 1, GRDMA_H2_META_ERR_STREAM = 2, GRDMA_H2_META_ERR_STRING = 3 };
enum grdma_h2_meta_kind { GRDMA_H2_META_REQUEST = 1, GRDMA_H2_META_RESPONSE = 2, GRDMA_H2_META_TRAILERS = 3 };
enum grdma_h2_meta_verdict {
  GRDMA_H2_META_OK = 0, GRDMA_H2_META_MALFORMED = 1, GRDMA_H2_META_BAD_METHOD = 2, GRDMA_H2_META_BAD_CONTENT_TYPE = 3, GRDMA_H2_META_BAD_TE = 4,
  GRDMA_H2_META_BAD_TIMEOUT = 5, GRDMA_H2_META_UNIMPLEMENTED = 6, GRDMA_H2_META_BAD_ENCODING = 7, GRDMA_H2_META_HTTP_STATUS = 8,
  GRDMA_H2_META_NO_STATUS = 9, GRDMA_H2_META_BAD_GRPC_STATUS = 10
};
enum grdma_h2_meta_call_flag {
  GRDMA_H2_META_HAS_TIMEOUT = 1, GRDMA_H2_META_END_STREAM = 2, GRDMA_H2_META_HAS_GRPC_STATUS = 4, GRDMA_H2_META_HAS_MESSAGE = 8
};
typedef struct grdma_h2_call_meta {   /* 48 bytes, one per input block, in block order */
  uint32_t stream;
  uint32_t word;          /* kind (bits 0..7) | verdict << 8 | encoding << 16 | flags << 24 */
  uint32_t method;        /* index into the create-time path list, 0xffffffff: none */
  uint32_t http_status;   /* :status as a number, 0xffffffff: none */
  uint32_t grpc_status;   /* grpc-status as a number, 0xffffffff: none */
  uint32_t timeout_lo, timeout_hi;   /* nanoseconds, saturated at 2^63 - 1; 0 without HAS_TIMEOUT */
  uint32_t path_field, authority_field, message_field;  /* index into the FIELD TABLE, 0xffffffff: none */
  uint32_t ncustom;       /* fields whose name is none of the known keys */
  uint32_t bad_field;     /* index into the field table of the first field (block order) that made the block MALFORMED, else none */
} grdma_h2_call_meta;
typedef struct grdma_h2_meta grdma_h2_meta;
grdma_h2_meta* grdma_h2_meta_create(const void* methods, uint64_t methods_bytes, uint32_t nmethods, uint32_t accept_encodings);
void grdma_h2_meta_destroy(grdma_h2_meta* meta);
int64_t grdma_h2_meta_read(grdma_h2_meta* meta, const grdma_h2_header_block* d_blocks, uint64_t nblocks,
                           const grdma_h2_header_field* d_fields, uint64_t nfields, const void* d_strings, uint64_t strings_bytes,
                           grdma_h2_call_meta* d_meta, uint64_t meta_cap, grdma_h2_header_block* d_reject, uint64_t reject_cap,
                           uint64_t out[8]);  /* returns the number of rejection blocks */
/* {device address of the constant field table, its fields, device address of its string arena, its bytes}: valid until
 * the reader is destroyed */
int grdma_h2_meta_reject_tables(grdma_h2_meta* meta, uint64_t out[4]);
typedef struct grdma_h2_meta_item {      /* 80 bytes, every member 8 bytes wide: one link's input and targets, as grdma_h2_meta_read's */
  const grdma_h2_header_block* d_blocks; uint64_t nblocks;
  const grdma_h2_header_field* d_fields; uint64_t nfields;
  const void* d_strings;                 uint64_t strings_bytes;
  grdma_h2_call_meta* d_meta;            uint64_t meta_cap;
  grdma_h2_header_block* d_reject;       uint64_t reject_cap;
} grdma_h2_meta_item;
int grdma_h2_meta_read_batch(grdma_h2_meta* meta, const grdma_h2_meta_item* items, uint32_t n_items, uint64_t* out /* 8 words per item */);
/* {calls, blocks, requests, responses, trailers, rejections, malformed, kernel time of the last call in NANOseconds (HIP
 * events)} */
int grdma_h2_meta_stats(grdma_h2_meta* meta, uint64_t out[8]);

/* ---- Call table: per-call state on the device, messages routed by method (csrc/grdma_h2_calls.h) ----
 * One table per connection, resident in HBM, keyed by stream.  A STEP joins it with three device tables the earlier
 * stages wrote -- the call records of grdma_h2_meta_read (record k belongs to block k of the decoder's block table), the
 * received-message descriptors of grdma_h2_deframe_messages and the deframer's events -- and writes the DISPATCH TABLE,
 * the messages sorted by registered method so that a handler kernel for method m takes d_segments[m] ..
 * d_segments[m + 1] and nothing else, and the DONE LIST (deadlines that passed, streams that closed).  The table
 * belongs to no parser; every input and output is passed by address.  A step is ordered on the stream of the standalone
 * HTTP/2 calls: a grdma_h2_deframe_messages, grdma_h2_hpack_decode and grdma_h2_meta_read in front of it need no host
 * synchronisation beyond the counts the host already has (grdma_h2_asm_last_call names the assembler's tables).  The
 * sequential reference, which defines the exact output, is tests/h2_calls_model.py.
 * CREATE.  table_slots: a power of two in 16 .. 65536, 0 = 4096; at most half may be live.  nmethods: 0 .. 4096, the
 * reader's.  Keys hash as everywhere: (id >> 1) & mask, linear probing.
 * A step runs rules 1 to 4 in this order -- the wire's own: on one stream HEADERS precede DATA, which precedes the
 * close, and HTTP/2 never reuses an id.
 * 1. OPEN.  A record opens a call when its kind is REQUEST, its verdict OK, the status byte of its block (flags bits
 *    8..15) 0 and its stream has no entry.  The entry: {serial = the next of a 64-bit counter that starts at 0, given in
 *    record order; method; encoding; deadline = now_ns + timeout saturated at 2^64 - 1, or 2^64 - 1 without HAS_TIMEOUT;
 *    0 messages; 0 bytes}.  Ignored: a REQUEST with another verdict or a non-zero status byte (refused); a stream that
 *    has an entry or comes a second time in the step, where the first wins whether it opened or was lost (duplicate);
 *    any other kind (RESPONSE and TRAILERS: the client side is not here).  An opening that would make more than
 *    table_slots / 2 entries live does not happen: the call is lost, the sticky flag GRDMA_H2_CALLS_LOST is set, the
 *    records in front of it are unaffected.
 * 2. EXPIRE.  A live entry not yet EXPIRED whose deadline is <= now_ns becomes EXPIRED, stays in the table and gets one
 *    DEADLINE record; one opened in this step with timeout 0 is included.
 * 3. MESSAGES, in descriptor order.  A descriptor is an ORPHAN, in this order of checks, when its status is not
 *    GRDMA_H2_MSG_OK (BAD_STATUS), its stream has no entry (NO_CALL), the entry is EXPIRED (EXPIRED), the compressed bit
 *    is set on encoding 0 (COMPRESSED_IDENTITY).  Every other descriptor is DISPATCHED to its entry's method: seq
 *    continues the entry's message count, the entry's messages and bytes grow.  A dispatch record: offset and length
 *    are the descriptor's, msg its index in d_msgs; word = flags | reason << 8 | encoding << 16.  Flags: FIRST (a
 *    dispatched record whose seq is 0), LAST (the last DISPATCHED message of its stream in this step, when the step
 *    holds a STREAM_CLOSED event of the stream with a of 0 or 1), COMPRESSED (bit 0 of the descriptor's flags).  An
 *    orphan has method 0xffffffff, seq 0, neither FIRST nor LAST; call and encoding are its entry's where the entry was
 *    looked at (EXPIRED, COMPRESSED_IDENTITY) and 0 otherwise.
 * 4. CLOSE, in event order, over the events of kind STREAM_CLOSED (7) whose stream (word c) has an entry.  a == 0: the
 *    entry becomes READS_CLOSED, one READS_CLOSED record.  a == 1: one LEFT record, the entry is removed (a later event
 *    of the stream finds no entry).  No other event is read, nor a STREAM_CLOSED with another a.  A done record's word is
 *    reason | flags << 8, the flag WAS_READS_CLOSED on a LEFT or DEADLINE record of an entry that was READS_CLOSED;
 *    messages and bytes are the call's dispatched messages since it opened, this step's included.
 * 5. THE DONE LIST holds the DEADLINE records first, in ascending stream order, then the close records in event order.
 * 6. THE DISPATCH TABLE is sorted by method, stable in descriptor order, the orphans behind the last method.
 *    d_segments has nmethods + 2 words: [m] .. [m + 1] is method m's list, index nmethods the orphans', [nmethods + 1]
 *    the total.
 * 7. BAD INPUT is found on the device: a record that meets the first three conditions of rule 1 with a stream of 0 or
 *    above 2^31 - 1 (ERR_STREAM) or a method >= nmethods (ERR_METHOD); the first such record in record order, in it
 *    the stream first.  Result word 6 is BAD_INPUT | code << 8 | record << 32, the other words are 0, nothing is
 *    written, nothing is committed, the call returns -GRDMA_ERR_INVALID.  Not sticky.
 * 8. CAPS.  dispatch_cap < nmsgs or done_cap < the done records: overflow word 1, -GRDMA_ERR_CAPACITY, the result block
 *    holds the totals, NOTHING is written to any target (d_segments included) and NOTHING is committed: not the table,
 *    the serial counter, the counters or the LOST flag.  The same step with larger targets gives what a never-refused
 *    step gives.  Nothing is written behind the totals in any case; d_segments is written whole.
 * 9. RESULT BLOCK: {opened, dispatched, orphans, done records, expired in this step, live entries after the step, flags
 *    (grdma_h2_calls_flag) | error << 8 | record << 32, overflow}.  grdma_h2_calls_step returns the number of dispatch
 *    records (= nmsgs).  STATS: {steps, opened, dispatched messages, dispatched bytes, orphans, done records, the LOST
 *    flag, kernel time of the last step in NANOseconds}.  DUMP: the live entries, sorted by stream, 48 bytes each
 *    (grdma_h2_call_entry); out = {entries, bytes, the serial counter, table_slots}; -GRDMA_ERR_CAPACITY with out filled
 *    in when cap is too small.
 * 10. -GRDMA_ERR_INVALID (grdma_last_error says why; nothing runs, nothing changes): null, zero-cap or misaligned (16
 *    bytes) targets, a null input table with a count above 0, nmsgs above 2^20, 2^32 - 1 records or events or more, no
 *    table, no result array.
 * A step is eight launches whatever the counts; its call words go up in one copy, its result words come down in one.
 * MANY LINKS.  grdma_h2_calls_step_batch is grdma_h2_calls_step for n items (1 .. GRDMA_H2_BATCH_MAX) in eight launches
 * however many (k_h2_links_calls_*), ordered on the same stream: a grdma_h2_hpack_decode_batch and a
 * grdma_h2_meta_read_batch in front of it need no host synchronisation beyond the counts the host already has.  n tables,
 * one item each, by design (unlike the metadata reader, which is one object for all links): a table's state is per
 * connection, as the header encoder's, so an item is a table and the thirteen arguments of the single step behind it.
 *  1. Every item is stepped by rules 1 to 9 exactly as the single call steps it: its dispatch table, its segment words,
 *     its done list, its eight result words, its table (the dump) and its counters are byte for byte what
 *     grdma_h2_calls_step gives that table for the same arguments.
 *  2. Single and batch steps may alternate on one table.
 *  3. now_ns is per item.
 *  4. Input tables may be shared between items; overlapping targets are the caller's error and are not checked.
 *  5. Trouble stays with its item, the other items are exact.  Bad input (rule 7): the flag, the code and the record in
 *     the item's word 6, its other words 0, nothing is written or committed for that table.  A cap overflow (rule 8):
 *     overflow word 1 and the totals, nothing is written or committed.  Repeated alone or in a later batch with larger
 *     targets the item gives what a never-refused step gives.  The sticky LOST flag behaves per table as in the single
 *     call.
 *  6. An item with no records, messages or events is still a step: it commits, `steps` moves, EXPIRE runs against its
 *     now_ns.
 *  7. The return value is the number of items that committed (overflow word 0 and no BAD_INPUT), or a negative error.
 *     out: 8 result words per item, in item order.
 *  8. -GRDMA_ERR_INVALID (grdma_last_error says why; nothing runs, nothing changes, out is not touched): n outside 1 ..
 *     GRDMA_H2_BATCH_MAX, a NULL item array or result array, an item without table, the same table twice, any item the
 *     single call's argument checks (rule 10) refuse.
 *  9. COUNTERS are per table: a committed item moves its table's grdma_h2_calls_stats as one single step would, an item
 *     that did not commit moves nothing.  Word 7 of every table in the batch is the batch's kernel time.
 * All items' call words go up in ONE copy and all result words come down in ONE copy, whatever n; no table needs device
 * memory for the batch beyond what its single steps use.
 * Not here: the table inside a pipe or group pipe, a grid per link sized by the link's counts, the client side
 * (RESPONSE and TRAILERS records are ignored), RST_STREAM for malformed or expired calls, reporting finished replies to
 * grdma_h2_parser_close_writes, decompression. */
enum grdma_h2_calls_flag { GRDMA_H2_CALLS_BAD_INPUT = 1, GRDMA_H2_CALLS_LOST = 2 };
enum grdma_h2_calls_error { GRDMA_H2_CALLS_ERR_STREAM = 1, GRDMA_H2_CALLS_ERR_METHOD = 2 };
enum grdma_h2_dispatch_flag { GRDMA_H2_DISPATCH_FIRST = 1, GRDMA_H2_DISPATCH_LAST = 2, GRDMA_H2_DISPATCH_COMPRESSED = 4 };
enum grdma_h2_orphan_reason {
  GRDMA_H2_ORPHAN_NO_CALL = 1, GRDMA_H2_ORPHAN_EXPIRED = 2, GRDMA_H2_ORPHAN_BAD_STATUS = 3, GRDMA_H2_ORPHAN_COMPRESSED_IDENTITY = 4
};
enum grdma_h2_done_reason { GRDMA_H2_DONE_READS_CLOSED = 1, GRDMA_H2_DONE_LEFT = 2, GRDMA_H2_DONE_DEADLINE = 3 };
enum grdma_h2_done_flag { GRDMA_H2_DONE_WAS_READS_CLOSED = 1 };
enum grdma_h2_call_entry_flag { GRDMA_H2_CALL_READS_CLOSED = 1, GRDMA_H2_CALL_EXPIRED = 2 };
typedef struct grdma_h2_dispatch {    /* 48 bytes */
  uint64_t offset, length;            /* the descriptor's */
  uint64_t call;                      /* the call's serial */
  uint32_t stream;
  uint32_t msg;                       /* index of the descriptor in d_msgs */
  uint32_t method;                    /* 0xffffffff in the orphan segment */
  uint32_t word;                      /* flags | reason << 8 | encoding << 16 */
  uint32_t seq;                       /* number of this message within its call, from 0 */
  uint32_t pad;
} grdma_h2_dispatch;
typedef struct grdma_h2_call_done {   /* 32 bytes */
  uint64_t call, bytes;
  uint32_t stream, method, messages;
  uint32_t word;                      /* reason | flags << 8 */
} grdma_h2_call_done;
typedef struct grdma_h2_call_entry {  /* 48 bytes: a dumped entry */
  uint64_t call, deadline_ns, bytes;
  uint32_t stream, method, messages;
  uint32_t word;                      /* encoding | flags << 8 (grdma_h2_call_entry_flag) */
  uint32_t pad[2];
} grdma_h2_call_entry;
typedef struct grdma_h2_calls grdma_h2_calls;
grdma_h2_calls* grdma_h2_calls_create(uint32_t table_slots, uint32_t nmethods);
void grdma_h2_calls_destroy(grdma_h2_calls* calls);
int64_t grdma_h2_calls_step(grdma_h2_calls* calls, const grdma_h2_header_block* d_blocks, const grdma_h2_call_meta* d_meta, uint64_t nblocks,
                            const grdma_h2_rx_msg* d_msgs, uint64_t nmsgs, const grdma_h2_event* d_events, uint64_t nevents,
                            uint64_t now_ns, grdma_h2_dispatch* d_dispatch, uint64_t dispatch_cap, uint32_t* d_segments,
                            grdma_h2_call_done* d_done, uint64_t done_cap, uint64_t out[8]);
typedef struct grdma_h2_calls_item {     /* 112 bytes, every member 8 bytes wide: a table and its step's arguments, as grdma_h2_calls_step's */
  grdma_h2_calls* calls;
  const grdma_h2_header_block* d_blocks; const grdma_h2_call_meta* d_meta; uint64_t nblocks;
  const grdma_h2_rx_msg* d_msgs;         uint64_t nmsgs;
  const grdma_h2_event* d_events;        uint64_t nevents;
  uint64_t now_ns;
  grdma_h2_dispatch* d_dispatch;         uint64_t dispatch_cap;
  uint32_t* d_segments;
  grdma_h2_call_done* d_done;            uint64_t done_cap;
} grdma_h2_calls_item;
int grdma_h2_calls_step_batch(const grdma_h2_calls_item* items, uint32_t n_items, uint64_t* out /* 8 words per item */);
int grdma_h2_calls_dump(grdma_h2_calls* calls, void* host_buf, uint64_t cap, uint64_t out[4]);
int grdma_h2_calls_stats(grdma_h2_calls* calls, uint64_t out[8]);
/* {device address of the descriptors of the assembler's last grdma_h2_deframe_messages, their number, device address of
 * its parser's event list, its number of events}: valid until that parser's next deframing (both numbers are 0 behind a
 * call whose events or descriptors overflowed).  -GRDMA_ERR_INVALID on an assembler attached to a pipe. */
int grdma_h2_asm_last_call(grdma_h2_asm* a, uint64_t out[4]);

/* ---- HTTP/2 on several links of ONE job (the group pipe) ----
 * grdma_h2_pipe serves one link, and a job carries one set of kernels in front of and behind its rounds: a second
 * grdma_h2_pipe on another link of the same job replaces the first one's.  The group pipe is the pipe of n links of a
 * multi-link job (up to GRDMA_H2_BATCH_MAX): a step rewrites the slice tables of the listed links from their message
 * tables (k_h2_frame_links, ONE kernel for all of them), the job carries all its links, and the listed links' delivered
 * slices are parsed (k_h2_deframe_links, ONE kernel) -- by default both inside the job's graph, one launch per step
 * however many links; with GRDMA_H2_PIPE_FUSED=0 enqueued around the launch, with per-stage timing.  Links that are
 * not listed are carried as before, their tables untouched.  Both directions of a bidirectional pair are two specs
 * with two parsers.  The job has run once; delivered_slices is what that run delivered on the link.  A step parses
 * what THAT step delivered: the deframing kernel reads the count the job's drain leaves on the device (at small rings
 * a step starts at another ring phase than the recorded run and may deliver a slice more or less), and
 * grdma_h2_group_pipe_sync's "slices parsed" word is that count.  (grdma_h2_pipe parses the recorded count.)
 * Create returns NULL (grdma_last_error says why) for: n == 0, a link index out of range or listed twice, a parser
 * listed twice, nmsgs 0 or above 4096, max_frame 0 or >= 2^24, a job that already carries such kernels (another pipe).
 * Not here (yet): the chunked deframer inside the batch (every transport is parsed sequentially), the header encoder and the
 * header decoder inside the group pipe (standalone: grdma_h2_hpenc, and grdma_h2_hpack for one transport or many links, above).  A parser
 * that has a window ledger at create time is refused: ledgers come later, grdma_h2_group_pipe_attach_flow_control. */
typedef struct grdma_h2_link_spec {
  uint32_t link;                 /* index into the job's links; distinct */
  const grdma_h2_msg* msgs;
  uint64_t nmsgs;                /* 1 .. 4096 */
  grdma_h2_parser* parser;       /* distinct */
  uint64_t delivered_slices;     /* of this link in the recorded run */
  uint64_t events_cap;
} grdma_h2_link_spec;
typedef struct grdma_h2_group_pipe grdma_h2_group_pipe;
grdma_h2_group_pipe* grdma_h2_group_pipe_create(grdma_stream_job* job, const grdma_h2_link_spec* specs, uint32_t n,
                                                uint32_t max_frame);
int grdma_h2_group_pipe_enqueue(grdma_h2_group_pipe* p);
/* waits for the last step; out: 14 words per spec, the words of grdma_h2_pipe_sync (the two timing words are the
 * batch's, repeated); -GRDMA_ERR_INVALID when out_words < 14 n */
int grdma_h2_group_pipe_sync(grdma_h2_group_pipe* p, uint64_t* out, uint64_t out_words);
/* the events of spec i in the last step: their number, or -GRDMA_ERR_CAPACITY if more than cap */
int64_t grdma_h2_group_pipe_events(grdma_h2_group_pipe* p, uint32_t i, grdma_h2_event* out, uint64_t cap);
/* the slice table the job sends from on spec i's link, as grdma_h2_pipe_slice_table */
int64_t grdma_h2_group_pipe_slice_table(grdma_h2_group_pipe* p, uint32_t i, grdma_slice* out, uint64_t cap);
/* grdma_h2_pipe_attach_assembler for the group pipe: every later step assembles the messages of the listed links
 * behind k_h2_deframe_links -- six more kernels (k_h2_asm_*_links) however many links, inside the job's graph when the
 * pipe is fused (1 kernel in front, 1 + 6 behind), else enqueued behind the deframing on the job's stream.  n is the
 * pipe's spec count; asms[i] belongs to spec i's parser, NULL = that link stays without.  A step first releases
 * everything its assemblers reported before it.  While attached, grdma_h2_asm_release, grdma_h2_asm_release_batch and
 * both batch calls refuse the assembler and grdma_h2_asm_destroy does nothing: destroy the pipe first.
 * -GRDMA_ERR_INVALID (pipe and job as before): n other than the spec count, all entries NULL, an assembler of another
 * parser than its spec's, one attached anywhere already, one listed twice, a second attach. */
int grdma_h2_group_pipe_attach_assemblers(grdma_h2_group_pipe* p, grdma_h2_asm* const* asms, uint32_t n);
/* the descriptors of spec i in the last synced step, as grdma_h2_pipe_messages: their number, -GRDMA_ERR_CAPACITY if
 * more than cap, -GRDMA_ERR_INVALID for a spec without assembler */
int64_t grdma_h2_group_pipe_messages(grdma_h2_group_pipe* p, uint32_t i, grdma_h2_rx_msg* out, uint64_t cap);
/* grdma_h2_pipe_attach_flow_control for the group pipe: every later step accounts the events of the listed links --
 * five more kernels (k_h2_links_fc_*) however many links, behind the deframing and in attach order with the
 * assemblers' six (grdma_job_hook_counts = (1, 6), (1, 12) with assemblers; with GRDMA_H2_PIPE_FUSED=0 enqueued behind
 * the deframing).  n is the pipe's spec count; fcs[i] belongs to spec i's parser, NULL = that link stays without.  The
 * pipe owns each listed link's window-update list (room for that ledger's max_updates frames).  ORDER: the create calls
 * refuse a parser that already has a ledger, so create the pipe first, then grdma_h2_fc_create on the link's parser,
 * then attach.  While attached, grdma_h2_fc_account, grdma_h2_fc_account_batch and grdma_h2_pipe_attach_flow_control
 * refuse the ledger and grdma_h2_fc_destroy does nothing: destroy the pipe first (that detaches it).
 * -GRDMA_ERR_INVALID (pipe and job as before): n other than the spec count, all entries NULL, a ledger of another
 * parser than its spec's, one attached anywhere already, one listed twice, one whose parser is gone, a second attach, a
 * group reply pipe (not built). */
int grdma_h2_group_pipe_attach_flow_control(grdma_h2_group_pipe* p, grdma_h2_fc* const* fcs, uint32_t n);
/* the window-update list of spec i in the last step, as grdma_h2_pipe_window_updates / _window_update_bytes;
 * -GRDMA_ERR_INVALID for a spec without ledger */
int64_t grdma_h2_group_pipe_window_updates(grdma_h2_group_pipe* p, uint32_t i, grdma_slice* slices_out, uint64_t cap,
                                           uint64_t out[8]);
int64_t grdma_h2_group_pipe_window_update_bytes(grdma_h2_group_pipe* p, uint32_t i, void* bytes_out, uint64_t cap);
/* removes the kernels from the job's graph, detaches the assemblers, unbinds the replies of a group reply pipe; does
 * nothing while a reply pipe or group reply pipe reads one of this pipe's assemblers: destroy that one first */
void grdma_h2_group_pipe_destroy(grdma_h2_group_pipe* p);

/* grdma_h2_pipe_create_reply for n links of ONE back job: a group pipe whose framing stage is the listed replies --
 * k_h2_reply_plan_links and k_h2_reply_emit_links, two kernels in front of the job's rounds however many links
 * (grdma_job_hook_counts = (2, 1), (2, 7) with assemblers attached on the back side; with GRDMA_H2_PIPE_FUSED=0
 * enqueued in front of the launch inside the framing timing events).  A step frames, per link, what the LAST ENQUEUED
 * step of that reply's forward pipe or forward group pipe reported, sends it over the link and deframes it with
 * parser_back.  The object is grdma_h2_group_pipe: enqueue, sync, events, slice_table, attach_assemblers, messages and
 * destroy work on it unchanged.  job_back has run once over slice lists of the lengths the replies will have;
 * delivered_slices and recorded_wire_bytes are that run's per link.  The shape is checked PER LINK: a link whose step
 * has another slice count or other wire bytes writes nothing and re-sends its previous table, and sync reports frame
 * overflow 2 for that spec only; the other links of the step are framed, sent and parsed as usual.  Ordering is by
 * events: the step waits for every distinct source parser's last deframing, and a forward step's release (single pipe
 * or group pipe) waits for the last reply step that gathers from its arena.  grdma_h2_pipe_destroy and
 * grdma_h2_group_pipe_destroy of a forward pipe do nothing while this pipe reads one of its assemblers: destroy this
 * one first, then the forward pipes, then the replies.
 * NULL (grdma_last_error says why) for: what grdma_h2_group_pipe_create refuses of job, n, links and parsers, a NULL
 * reply, a reply listed twice or bound to a pipe already, a source assembler that is not attached to a forward pipe,
 * a job that already carries hooks. */
typedef struct grdma_h2_reply_link_spec {
  uint32_t link;                  /* index into job_back's links; distinct */
  grdma_h2_reply* reply;          /* distinct, not bound; its source assembles in a forward pipe or group pipe */
  grdma_h2_parser* parser_back;   /* distinct */
  uint64_t delivered_slices;      /* of this link in the recorded run */
  uint64_t events_cap;
  uint64_t recorded_wire_bytes;   /* what the recorded run sent on this link */
} grdma_h2_reply_link_spec;
grdma_h2_group_pipe* grdma_h2_group_pipe_create_reply(grdma_stream_job* job_back,
                                                      const grdma_h2_reply_link_spec* specs, uint32_t n);

/* ---- GRPCProfiler: include/grpcpp/stats_time.h:11-44,111-122, src/core/lib/debug/stats_time.cc ----
 * The reference's scope profiler with its op names in its order: nanoseconds per op per thread slot,
 * opt-in per thread (init(slot) + enable()), the table {Name, Count, Mean, P50, P95, P99, MAX} per slot
 * in the unit GRPC_PROFILING_UNIT names (micro / milli / s).  The host layer records
 * TRANSPORT_{READ,HANDLE_READ,CONTINUE_READ,DO_READ,FLUSH,HANDLE_WRITE,WRITE} in the endpoint mirror
 * and PAIR_SEND / PAIR_RECV around Send / Recv, where rdma_bp_posix.cc and pair.cc place their
 * GRPCProfiler objects.  Host only (no device needed). */
typedef enum grdma_stats_time {
  GRDMA_STATS_TIME_POLLABLE_EPOLL,
  GRDMA_STATS_TIME_POLLSET_WORK,
  GRDMA_STATS_TIME_TRANSPORT_DO_READ,
  GRDMA_STATS_TIME_TRANSPORT_CONTINUE_READ,
  GRDMA_STATS_TIME_TRANSPORT_READ_ALLOCATION_DONE,
  GRDMA_STATS_TIME_TRANSPORT_HANDLE_READ,
  GRDMA_STATS_TIME_TRANSPORT_READ,
  GRDMA_STATS_TIME_TRANSPORT_FLUSH,
  GRDMA_STATS_TIME_TRANSPORT_HANDLE_WRITE,
  GRDMA_STATS_TIME_TRANSPORT_WRITE,
  GRDMA_STATS_TIME_PAIR_SEND,
  GRDMA_STATS_TIME_PAIR_RECV,
  GRDMA_STATS_TIME_CLIENT_PREPARE,
  GRDMA_STATS_TIME_CLIENT_CQ_NEXT,
  GRDMA_STATS_TIME_SERVER_RPC_REQUEST,
  GRDMA_STATS_TIME_SERVER_RPC_FINISH,
  GRDMA_STATS_TIME_SERVER_CQ_NEXT,
  GRDMA_STATS_TIME_BEGIN_WORKER,
  GRDMA_STATS_TIME_ASYNC_NEXT_INTERNAL,
  GRDMA_STATS_TIME_FINALIZE_RESULT,
  GRDMA_STATS_TIME_DESERIALIZE,
  GRDMA_STATS_TIME_ADHOC_1,
  GRDMA_STATS_TIME_ADHOC_2,
  GRDMA_STATS_TIME_ADHOC_3,
  GRDMA_STATS_TIME_ADHOC_4,
  GRDMA_STATS_TIME_ADHOC_5,
  GRDMA_STATS_TIME_ADHOC_6,
  GRDMA_STATS_TIME_ADHOC_7,
  GRDMA_STATS_TIME_ADHOC_8,
  GRDMA_STATS_TIME_ADHOC_9,
  GRDMA_STATS_TIME_ADHOC_10,
  GRDMA_STATS_TIME_MAX_OP_SIZE
} grdma_stats_time;
void grdma_stats_time_init(int slot);          /* grpc_stats_time_init: the calling thread records into `slot` */
void grdma_stats_time_enable(void);
void grdma_stats_time_disable(void);
int grdma_stats_time_enabled(void);            /* enabled AND the calling thread has a slot */
void grdma_stats_time_shutdown(void);
void grdma_stats_time_add(int op, int64_t ns);          /* grpc_stats_time_add */
void grdma_stats_time_add_custom(int op, int64_t val);  /* grpc_stats_time_add_custom: printed unscaled */
const char* grdma_stats_time_op_name(int op);           /* grpc_stats_time_op_to_str */
int64_t grdma_stats_time_now_ns(void);
/* {mean, p50, p95, p99, max} in ns of one op of one slot; returns the count */
uint64_t grdma_stats_time_get(int slot, int op, double out[5]);
/* grpc_stats_time_print into buf (NUL-terminated, truncated to cap); returns the full length */
int64_t grdma_stats_time_print(char* buf, uint64_t cap);

/* ---- device helpers for callers that keep payloads in HBM ---------------------- */
void* grdma_device_alloc(uint64_t bytes);
void grdma_device_free(void* p);
/* Binds every thread of the process (and the threads started later) to the CPUs of the NUMA node the device hangs on,
 * the way `numactl --cpunodebind` would: pinned buffers allocated afterwards and the polling threads sit next to the
 * device's PCIe root.  Returns the node, or -1 when it is unknown (nothing changed then). */
int grdma_host_pin_to_device_node(void);
/* Binds the CALLING thread alone to the k-th physical core of that node, counted from the end of the node's CPU list
 * (`taskset -c`): busy-polling threads of one process then never share a core's two hardware threads.  Returns the CPU,
 * or -1 (nothing changed). */
int grdma_host_pin_thread_to_core(int k);
void* grdma_host_alloc_pinned(uint64_t bytes);
void grdma_host_free_pinned(void* p);
int grdma_copy_to_device(void* dst, const void* src, uint64_t n);
int grdma_copy_to_host(void* dst, const void* src, uint64_t n);
int grdma_device_synchronize(void);

#ifdef __cplusplus
}
#endif
#endif /* GRDMA_AMD_H */
