"""The C ABI of include/grdma_amd.h as ctypes sees it: one Structure per header struct the Python side fills or reads,
and one prototype per function the header declares.  _lib.load() applies the tables; tests/test_abi_table.py holds both
to the header (return and parameter classes, struct sizes, field offsets and field names).

Pointer parameters that take device addresses or opaque handles are c_void_p; a typed POINTER marks host arrays and
out-parameters, so a call that passes the wrong object fails in ctypes rather than in the library."""
import ctypes as C

P = C.POINTER
vp, cstr = C.c_void_p, C.c_char_p
i32, u32, i64, u64, f64, u8 = C.c_int, C.c_uint32, C.c_int64, C.c_uint64, C.c_double, C.c_uint8


class Slice(C.Structure):
    _fields_ = [("ptr", vp), ("len", u64)]


class ReadSlice(C.Structure):
    _fields_ = [("off", u64), ("len", u64)]


class PairState(C.Structure):
    _fields_ = [(n, u64) for n in (
        "head", "moving_head", "remain", "remote_tail", "remote_head", "internal_read_size",
        "credit_msgs", "partial_write", "total_read", "total_written", "leftover_cap")]


class Config(C.Structure):
    _fields_ = [("device_name", C.c_char * 64), ("port_num", i32), ("gid_index", i32),
                ("poller_thread_num", i32), ("busy_polling_timeout_us", i32),
                ("poller_sleep_timeout_ms", i32), ("ring_buffer_size_kb", u32),
                ("zerocopy_buffer_size_kb", u32), ("zerocopy_threshold_kb", u32),
                ("max_sge", i32), ("hip_device", i32), ("hip_wire_direct", i32),
                ("hip_register_min", u32), ("hip_pair_pool_mb", u32)]


class StreamResult(C.Structure):
    _fields_ = [(n, u64) for n in ("bytes_sent", "bytes_delivered", "slices_delivered",
                                   "tx_rounds", "rx_rounds", "tx_records", "rx_records", "done")] + \
               [("ms_total", f64), ("ms_class", f64 * 8), ("launches_class", u64 * 8)]


class H2Msg(C.Structure):
    _fields_ = [("payload", vp), ("len", u64), ("stream_id", u32), ("flags", u32)]


class H2Event(C.Structure):
    _fields_ = [(n, u32) for n in ("kind", "a", "b", "c", "d", "slice")]


class H2RxMsg(C.Structure):
    _fields_ = [("offset", u64), ("length", u64), ("seq", u64), ("stream_id", u32), ("status", u32),
                ("flags", u32), ("pad", u32)]


class H2Route(C.Structure):
    _fields_ = [("from_stream", u32), ("to_stream", u32)]


class H2DeframeItem(C.Structure):
    _fields_ = [("parser", vp), ("d_arena", vp), ("slices", P(ReadSlice)), ("n", u64),
                ("events_out", P(H2Event)), ("cap", u64), ("n_events", i64), ("h2_error", i32)]


class H2MessagesItem(C.Structure):
    _fields_ = H2DeframeItem._fields_ + [("assembler", vp), ("msgs_out", P(H2RxMsg)), ("msgs_cap", u64),
                                         ("n_msgs", i64)]


class H2LinkSpec(C.Structure):
    _fields_ = [("link", u32), ("msgs", P(H2Msg)), ("nmsgs", u64), ("parser", vp),
                ("delivered_slices", u64), ("events_cap", u64)]


class H2ReplyItem(C.Structure):
    _fields_ = [("reply", vp), ("d_slices_out", vp), ("slices_cap", u64), ("d_hdr_arena", vp),
                ("hdr_cap", u64), ("out", u64 * 8), ("n_slices", i64)]


class H2ReplyLinkSpec(C.Structure):
    _fields_ = [("link", u32), ("reply", vp), ("parser_back", vp), ("delivered_slices", u64),
                ("events_cap", u64), ("recorded_wire_bytes", u64)]


class H2FcItem(C.Structure):
    _fields_ = [("fc", vp), ("d_slices_out", vp), ("slices_cap", u64), ("d_hdr_arena", vp), ("hdr_cap", u64)]


class H2SwFrameItem(C.Structure):
    _fields_ = [("sw", vp), ("msgs", P(H2Msg)), ("progress", P(u64)), ("nmsgs", u64),
                ("max_frame", u32), ("pad", u32), ("d_slices_out", vp), ("slices_cap", u64),
                ("d_hdr_arena", vp), ("hdr_cap", u64)]


class H2WrItem(C.Structure):
    _fields_ = [("reply", vp), ("flags", u32), ("pad", u32), ("d_slices_out", vp),
                ("slices_cap", u64), ("d_hdr_arena", vp), ("hdr_cap", u64), ("n_slices", i64),
                ("out", u64 * 16)]


class H2CtlItem(C.Structure):
    _fields_ = [("ctl", vp), ("d_slices_out", vp), ("slices_cap", u64), ("d_hdr_arena", vp), ("hdr_cap", u64)]


class H2HpackItem(C.Structure):
    _fields_ = [("hpack", vp), ("d_blocks", vp), ("blocks_cap", u64), ("d_fields", vp),
                ("fields_cap", u64), ("d_strings", vp), ("strings_cap", u64)]


class H2HpencItem(C.Structure):
    _fields_ = [("enc", vp), ("d_blocks", vp), ("nblocks", u64), ("d_fields", vp), ("nfields", u64),
                ("d_strings", vp), ("strings_bytes", u64), ("d_wire", vp), ("wire_cap", u64),
                ("d_block_wire", vp), ("block_wire_cap", u64)]


# ctypes class -> the header struct it mirrors
STRUCTS = {
    Slice: "grdma_slice", ReadSlice: "grdma_read_slice", PairState: "grdma_pair_state", Config: "grdma_config",
    StreamResult: "grdma_stream_result", H2Msg: "grdma_h2_msg", H2Event: "grdma_h2_event", H2RxMsg: "grdma_h2_rx_msg",
    H2Route: "grdma_h2_route", H2DeframeItem: "grdma_h2_deframe_item", H2MessagesItem: "grdma_h2_messages_item",
    H2LinkSpec: "grdma_h2_link_spec", H2ReplyItem: "grdma_h2_reply_item", H2ReplyLinkSpec: "grdma_h2_reply_link_spec",
    H2FcItem: "grdma_h2_fc_item", H2SwFrameItem: "grdma_h2_sw_frame_item", H2WrItem: "grdma_h2_wr_item",
    H2CtlItem: "grdma_h2_ctl_item", H2HpackItem: "grdma_h2_hpack_item", H2HpencItem: "grdma_h2_hpenc_item",
}

# name -> (restype, argtypes), one entry per function the header declares, in the header's order
SIGNATURES = {
    "grdma_parse_platform": (i32, [cstr]),
    "grdma_determine_platform": (i32, []),
    "grdma_config_from_env": (i32, [P(Config)]),
    "grdma_init": (i32, [i32]),
    "grdma_device_count": (i32, []),
    "grdma_last_error": (cstr, []),
    "grdma_abi_version": (i32, []),
    "grdma_pair_create": (vp, [u64, i32, i32]),
    "grdma_pair_connect": (i32, [vp, vp]),
    "grdma_pair_export_address": (i32, [vp, vp]),
    "grdma_pair_connect_remote": (i32, [vp, vp]),
    "grdma_pair_bootstrap_fd": (i32, [vp, i32]),
    "grdma_pair_disconnect": (i32, [vp]),
    "grdma_pair_destroy": (None, [vp]),
    "grdma_pair_pool_reserve": (i32, [u32, u64, i32, i32, u64]),
    "grdma_pair_pool_take": (vp, [cstr, u64, i32, i32]),
    "grdma_pair_pool_get": (vp, [cstr]),
    "grdma_pair_pool_putback": (None, [vp]),
    "grdma_pair_pool_stats": (i32, [P(u64)]),
    "grdma_pair_pool_trim": (None, []),
    "grdma_pair_get_status": (i32, [vp]),
    "grdma_pair_send": (i64, [vp, P(Slice), u64, u64, i32]),
    "grdma_pair_recv": (i64, [vp, vp, u64, i32]),
    "grdma_pair_has_message": (i32, [vp]),
    "grdma_pair_has_pending_writes": (i32, [vp]),
    "grdma_pair_readable_size": (i64, [vp]),
    "grdma_pair_writable_size": (i64, [vp]),
    "grdma_pair_enable_zerocopy": (i32, [vp, u64]),
    "grdma_pair_enable_zerocopy_ex": (i32, [vp, u64, i32]),
    "grdma_pair_zerocopy_mem": (i32, [vp]),
    "grdma_pair_allocate_send_buffer": (vp, [vp, u64]),
    "grdma_pair_send_zerocopy": (i64, [vp, P(Slice), u64, u64, i32]),
    "grdma_pair_zerocopy_state": (i32, [vp, P(u64)]),
    "grdma_pair_state_get": (i32, [vp, P(PairState)]),
    "grdma_pair_peek_ring": (i32, [vp, u64, vp, u64]),
    "grdma_pair_peek_staging": (i32, [vp, u64, vp, u64]),
    "grdma_pair_last_wrs": (i32, [vp, P((u64 * 2) * 2)]),
    "grdma_pair_ring_device_ptr": (vp, [vp]),
    "grdma_poller_create": (vp, [i32, i32]),
    "grdma_poller_destroy": (None, [vp]),
    "grdma_poller_add": (i32, [vp, vp]),
    "grdma_poller_remove": (i32, [vp, vp]),
    "grdma_poller_stats": (i32, [vp, P(u64), P(u64)]),
    "grdma_poller_threads": (i32, [vp]),
    "grdma_pair_get_wakeup_fd": (i32, [vp]),
    "grdma_pair_consume_wakeup": (i32, [vp]),
    "grdma_endpoint_write_begin": (i64, [vp, P(Slice), u64, i32]),
    "grdma_endpoint_write_step": (i64, [vp, P(i32)]),
    "grdma_endpoint_write_abort": (i32, [vp]),
    "grdma_endpoint_read": (i64, [vp, u64, P(ReadSlice), u64, P(i32)]),
    "grdma_endpoint_set_async": (i32, [vp, i32, u64]),
    "grdma_endpoint_write_submit": (i32, [vp]),
    "grdma_endpoint_write_test": (i32, [vp, P(i32), P(i64)]),
    "grdma_endpoint_write_queue": (i32, [vp, vp, u64]),
    "grdma_endpoint_write_adopt": (i32, [vp]),
    "grdma_endpoint_write_queue_stats": (i32, [vp, P(u64)]),
    "grdma_endpoint_write_queue_limits": (i32, [vp, P(u64)]),
    "grdma_endpoint_write_quiesce": (i32, [vp]),
    "grdma_endpoint_read_submit": (i32, [vp, u64]),
    "grdma_endpoint_read_test": (i64, [vp, vp, u64, vp, vp]),
    "grdma_endpoint_read_idle": (i32, [vp]),
    "grdma_endpoint_readable": (i32, [vp]),
    "grdma_endpoint_writable": (i32, [vp]),
    "grdma_endpoint_busy": (i32, [vp]),
    "grdma_endpoint_drain_state": (i32, [vp]),
    "grdma_endpoint_free_windows": (i32, [vp]),
    "grdma_window_base": (vp, [vp]),
    "grdma_window_ref": (None, [vp]),
    "grdma_window_unref": (None, [vp]),
    "grdma_set_host_register_min": (i32, [u64]),
    "grdma_forget_host_range": (i32, [vp, u64]),
    "grdma_pair_export_ring_dmabuf": (i32, [vp]),
    "grdma_verbs_supported": (i32, []),
    "grdma_pair_verbs_open": (i32, [vp, cstr, i32, i32]),
    "grdma_pair_verbs_address": (i32, [vp, vp]),
    "grdma_pair_verbs_connect": (i32, [vp, vp]),
    "grdma_pair_verbs_counts": (i32, [vp, P(u64)]),
    "grdma_pair_arena_device_ptr": (vp, [vp]),
    "grdma_pair_arena_size": (u64, [vp]),
    "grdma_pair_arena_copy_out": (i32, [vp, u64, vp, u64]),
    "grdma_pair_set_latency_mode": (i32, [vp, i32]),
    "grdma_pair_arm_read": (i32, [vp, u64]),
    "grdma_pair_watch_hits": (i64, [vp]),
    "grdma_engine_watchers": (i32, []),
    "grdma_pair_armed_ready": (i32, [vp]),
    "grdma_engine_start": (i32, []),
    "grdma_engine_stop": (i32, []),
    "grdma_pingpong": (i32, [vp, vp, P(Slice), u64, P(Slice), u64, i32, u64, u64, P(u64), P(u64)]),
    "grdma_pingpong_end": (i32, [vp, i32, P(Slice), u64, u64, i32, u64, u64, P(u64), P(u64)]),
    "grdma_poll_pairs": (i32, [P(vp), u32, P(u64), P(u8)]),
    "grdma_stream_job_create": (vp, [vp, vp, P(Slice), u64, vp, u64, u64, u64]),
    "grdma_stream_job_create_multi": (vp, [u32, P(vp), P(vp), P(Slice), P(u64), P(vp), P(u64), P(u64), u64]),
    "grdma_stream_job_slices_of": (i32, [vp, u32, P(ReadSlice), u64]),
    "grdma_stream_job_destroy": (None, [vp]),
    "grdma_stream_job_run": (i32, [vp, i32, P(StreamResult)]),
    "grdma_stream_job_launch": (i32, [vp]),
    "grdma_stream_job_launch_streams": (i32, [vp]),
    "grdma_stream_job_sync": (i32, [vp]),
    "grdma_stream_job_slices": (i32, [vp, P(ReadSlice), u64]),
    "grdma_stream_job_set_rounds": (i32, [vp, u64]),
    "grdma_stream_job_set_pipeline": (i32, [vp, i32]),
    "grdma_stream_job_set_sends": (i32, [vp, u32]),
    "grdma_stream_job_set_promised_credit": (i32, [vp, i32]),
    "grdma_stream_job_set_fused_wire": (i32, [vp, i32]),
    "grdma_stream_job_wire_groups": (u32, [vp]),
    "grdma_stream_job_set_rebuild_index": (i32, [vp, i32]),
    "grdma_pair_last_dbg": (i32, [vp, P(u64), P(u64)]),
    "grdma_stream_job_debug": (i32, [vp, P(u64), P(u64)]),
    "grdma_pair_debug_hist": (i32, [vp, P(u32), P(u64), P(u32)]),
    "grdma_engine_debug": (i32, [P(u64)]),
    "grdma_express_drains": (u64, []),
    "grdma_watch_fast_drains": (u64, []),
    "grdma_watch_ticks": (i32, [P(u64)]),
    "grdma_rx_express_ticks": (i32, [P(u64)]),
    "grdma_tx_fast_sends": (i32, [P(u64)]),
    "grdma_rx_fast_drains": (i32, [P(u64)]),
    "grdma_rx_table_cache_stats": (i32, [P(u64)]),
    "grdma_rx_verdict_counts": (i32, [P(u64)]),
    "grdma_debug_set_promise_wait": (i32, [u32]),
    "grdma_wire_wait_runouts": (u64, []),
    "grdma_tx_promise_counts": (i32, [P(u64)]),
    "grdma_tx_small_ticks": (i32, [P(u64)]),
    "grdma_host_free_size": (u64, [u64, u64, u64]),
    "grdma_host_writable": (u64, [u64, u64, u64]),
    "grdma_host_encoded_size": (u64, [u64]),
    "grdma_host_calc_writable": (u64, [u64]),
    "grdma_h2_frame_messages": (i64, [P(H2Msg), u64, u32, vp, u64, vp, u64, P(u64)]),
    "grdma_h2_parser_create": (vp, [i32, u32]),
    "grdma_h2_parser_create_ex": (vp, [i32, u32, u32, u32]),
    "grdma_h2_parser_destroy": (None, [vp]),
    "grdma_h2_parser_open_streams": (i32, [vp, P(u32), u32]),
    "grdma_h2_parser_close_writes": (i32, [vp, P(u32), u32]),
    "grdma_h2_parser_live_streams": (i64, [vp]),
    "grdma_h2_last_kernel_us": (f64, []),
    "grdma_h2_last_boundary_steps": (u64, []),
    "grdma_h2_last_deframe_stats": (None, [P(u64)]),
    "grdma_h2_parser_chunk_stats": (i32, [vp, P(u64)]),
    "grdma_h2_parser_chunk_dbg": (i32, [vp, P(u64), u64]),
    "grdma_h2_deframe": (i64, [vp, vp, P(ReadSlice), u64, P(H2Event), u64, P(i32)]),
    "grdma_h2_deframe_batch": (i32, [P(H2DeframeItem), u32]),
    "grdma_h2_pipe_create": (vp, [vp, u32, P(H2Msg), u64, u32, vp, u64, u64]),
    "grdma_h2_pipe_enqueue": (i32, [vp, i32]),
    "grdma_h2_pipe_sync": (i32, [vp, P(u64), P(H2Event), u64]),
    "grdma_h2_pipe_destroy": (None, [vp]),
    "grdma_h2_pipe_boundary_stats": (i32, [vp, P(u64)]),
    "grdma_h2_asm_create": (vp, [vp, vp, u64, u64, u32]),
    "grdma_h2_asm_destroy": (None, [vp]),
    "grdma_h2_deframe_messages": (i64, [vp, vp, vp, P(ReadSlice), u64, P(H2Event), u64, P(H2RxMsg), u64, P(i32)]),
    "grdma_h2_asm_release": (i32, [vp, u64]),
    "grdma_h2_asm_stats": (i32, [vp, P(u64)]),
    "grdma_h2_pipe_attach_assembler": (i32, [vp, vp]),
    "grdma_h2_pipe_messages": (i64, [vp, P(H2RxMsg), u64]),
    "grdma_h2_deframe_messages_batch": (i32, [P(H2MessagesItem), u32]),
    "grdma_h2_asm_release_batch": (i32, [P(vp), P(u64), u32]),
    "grdma_h2_reply_create": (vp, [vp, P(H2Route), u32, u32, u64]),
    "grdma_h2_reply_destroy": (None, [vp]),
    "grdma_h2_reply_frame": (i64, [vp, vp, u64, vp, u64, P(u64)]),
    "grdma_h2_reply_frame_batch": (i32, [P(H2ReplyItem), u32]),
    "grdma_h2_pipe_create_reply": (vp, [vp, u32, vp, vp, u64, u64, u64]),
    "grdma_h2_pipe_slice_table": (i64, [vp, P(Slice), u64]),
    "grdma_h2_fc_create": (vp, [vp, u32, u32, u32, u32]),
    "grdma_h2_fc_destroy": (None, [vp]),
    "grdma_h2_fc_account": (i64, [vp, vp, u64, vp, u64, P(u64)]),
    "grdma_h2_fc_stats": (i32, [vp, P(u64)]),
    "grdma_h2_pipe_attach_flow_control": (i32, [vp, vp]),
    "grdma_h2_pipe_window_updates": (i64, [vp, P(Slice), u64, P(u64)]),
    "grdma_h2_pipe_window_update_bytes": (i64, [vp, vp, u64]),
    "grdma_h2_fc_account_batch": (i32, [P(H2FcItem), u32, P(u64)]),
    "grdma_h2_sw_create": (vp, [vp, u32, u32, u32]),
    "grdma_h2_sw_destroy": (None, [vp]),
    "grdma_h2_sw_intake": (i64, [vp, P(u64)]),
    "grdma_h2_sw_frame": (i64, [vp, P(H2Msg), P(u64), u64, u32, vp, u64, vp, u64, P(u64)]),
    "grdma_h2_sw_windows": (i32, [vp, P(u32), u32, P(i64)]),
    "grdma_h2_sw_stats": (i32, [vp, P(u64)]),
    "grdma_h2_sw_intake_batch": (i32, [P(vp), u32, P(u64)]),
    "grdma_h2_sw_frame_batch": (i32, [P(H2SwFrameItem), u32, P(u64)]),
    "grdma_h2_reply_attach_windows": (i32, [vp, vp, u32]),
    "grdma_h2_reply_frame_windowed": (i64, [vp, u32, vp, u64, vp, u64, P(u64)]),
    "grdma_h2_reply_pending": (i64, [vp, P(u64), u64]),
    "grdma_h2_reply_frame_windowed_batch": (i32, [P(H2WrItem), u32]),
    "grdma_h2_ctl_create": (vp, [vp, u32]),
    "grdma_h2_ctl_destroy": (None, [vp]),
    "grdma_h2_ctl_reply": (i64, [vp, vp, u64, vp, u64, P(u64)]),
    "grdma_h2_ctl_peer": (i32, [vp, P(u64)]),
    "grdma_h2_ctl_stats": (i32, [vp, P(u64)]),
    "grdma_h2_ctl_reply_batch": (i32, [P(H2CtlItem), u32, P(u64)]),
    "grdma_h2_hpack_create": (vp, [vp, u32, u32]),
    "grdma_h2_hpack_destroy": (None, [vp]),
    "grdma_h2_hpack_set_max_table_size": (i32, [vp, u32]),
    "grdma_h2_hpack_decode": (i64, [vp, vp, u64, vp, u64, vp, u64, P(u64)]),
    "grdma_h2_hpack_table": (i32, [vp, vp, u64, P(u64)]),
    "grdma_h2_hpack_stats": (i32, [vp, P(u64)]),
    "grdma_h2_hpack_decode_batch": (i32, [P(H2HpackItem), u32, P(u64)]),
    "grdma_h2_hpenc_create": (vp, [u32, u32]),
    "grdma_h2_hpenc_destroy": (None, [vp]),
    "grdma_h2_hpenc_set_peer": (i32, [vp, u32, u32]),
    "grdma_h2_hpenc_encode": (i64, [vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64, P(u64)]),
    "grdma_h2_hpenc_table": (i32, [vp, vp, u64, P(u64)]),
    "grdma_h2_hpenc_stats": (i32, [vp, P(u64)]),
    "grdma_h2_hpenc_last_stages": (i32, [vp, P(u64)]),
    "grdma_h2_hpenc_encode_batch": (i32, [P(H2HpencItem), u32, P(u64)]),
    "grdma_h2_meta_create": (vp, [vp, u64, u32, u32]),
    "grdma_h2_meta_destroy": (None, [vp]),
    "grdma_h2_meta_read": (i64, [vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64, P(u64)]),
    "grdma_h2_meta_read_batch": (i32, [vp, vp, u32, P(u64)]),  # (the items: a (n, 10) array of 64-bit words, h2dev.META_ITEM)
    "grdma_h2_meta_reject_tables": (i32, [vp, P(u64)]),
    "grdma_h2_meta_stats": (i32, [vp, P(u64)]),
    "grdma_h2_calls_create": (vp, [u32, u32]),
    "grdma_h2_calls_destroy": (None, [vp]),
    "grdma_h2_calls_step": (i64, [vp, vp, vp, u64, vp, u64, vp, u64, u64, vp, u64, vp, vp, u64, P(u64)]),
    "grdma_h2_calls_step_batch": (i32, [vp, u32, P(u64)]),  # (the items: a (n, 14) array of 64-bit words, h2dev.CALLS_ITEM)
    "grdma_h2_calls_dump": (i32, [vp, vp, u64, P(u64)]),
    "grdma_h2_calls_stats": (i32, [vp, P(u64)]),
    "grdma_h2_asm_last_call": (i32, [vp, P(u64)]),
    "grdma_h2_group_pipe_create": (vp, [vp, P(H2LinkSpec), u32, u32]),
    "grdma_h2_group_pipe_enqueue": (i32, [vp]),
    "grdma_h2_group_pipe_sync": (i32, [vp, P(u64), u64]),
    "grdma_h2_group_pipe_events": (i64, [vp, u32, P(H2Event), u64]),
    "grdma_h2_group_pipe_slice_table": (i64, [vp, u32, P(Slice), u64]),
    "grdma_h2_group_pipe_attach_assemblers": (i32, [vp, P(vp), u32]),
    "grdma_h2_group_pipe_messages": (i64, [vp, u32, P(H2RxMsg), u64]),
    "grdma_h2_group_pipe_attach_flow_control": (i32, [vp, P(vp), u32]),
    "grdma_h2_group_pipe_window_updates": (i64, [vp, u32, P(Slice), u64, P(u64)]),
    "grdma_h2_group_pipe_window_update_bytes": (i64, [vp, u32, vp, u64]),
    "grdma_h2_group_pipe_destroy": (None, [vp]),
    "grdma_h2_group_pipe_create_reply": (vp, [vp, P(H2ReplyLinkSpec), u32]),
    "grdma_stats_time_init": (None, [i32]),
    "grdma_stats_time_enable": (None, []),
    "grdma_stats_time_disable": (None, []),
    "grdma_stats_time_enabled": (i32, []),
    "grdma_stats_time_shutdown": (None, []),
    "grdma_stats_time_add": (None, [i32, i64]),
    "grdma_stats_time_add_custom": (None, [i32, i64]),
    "grdma_stats_time_op_name": (cstr, [i32]),
    "grdma_stats_time_now_ns": (i64, []),
    "grdma_stats_time_get": (u64, [i32, i32, P(f64)]),
    "grdma_stats_time_print": (i64, [cstr, u64]),
    "grdma_device_alloc": (vp, [u64]),
    "grdma_device_free": (None, [vp]),
    "grdma_host_pin_to_device_node": (i32, []),
    "grdma_host_pin_thread_to_core": (i32, [i32]),
    "grdma_host_alloc_pinned": (vp, [u64]),
    "grdma_host_free_pinned": (None, [vp]),
    "grdma_copy_to_device": (i32, [vp, vp, u64]),
    "grdma_copy_to_host": (i32, [vp, vp, u64]),
    "grdma_device_synchronize": (i32, []),
}

# exported by the library and used by the tests of the HTTP/2 pipes (the job's side of a pipe: kernels in front of and
# behind the job's rounds inside its graph), but not part of include/grdma_amd.h
UNDECLARED = {
    "grdma_job_hook_counts": (i32, [vp, P(u32)]),
}
