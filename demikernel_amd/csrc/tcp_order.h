// tcp_order.h — what the calls on the two TCP data-plane contexts that live in other files than their context need of
// it. Of a dk_tcp_ctx (tcp_kernels.hip), for the calls that follow a dk_tcp_rx_process call on the same batch
// (dk_tcp_ack_process, tcp_ack_kernels.hip; dk_tcp_ack_emit, tcp_ackemit_kernels.hip; dk_tcp_cc_ack,
// tcp_cc_kernels.hip): the batch's order by connection, still in the context's buffers, the followers' own state, and
// the context's call order. Of a dk_tcp_tx_ctx (tcp_tx_kernels.hip): its call order and dk_tcp_tx_commit's state. The
// call order and the buffers are ctl_common.h's CallOrder and Buf. Internal to libdk_rx.so.
#ifndef DK_TCP_ORDER_H
#define DK_TCP_ORDER_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ctl_common.h"

struct dk_tcp_ctx;

struct dk_tcp_ack_state {
    int form = -1;       // dk_diag_tcp_ack_set_form: 0 lane, 1 wave, 2 chip, -1 the rule
    int last_form = -1;  // the form the last dk_tcp_ack_process call ran
    uint32_t done = 0;   // the dk_tcp_rx_process call number the last dk_tcp_ack_process call consumed
    dk::ctl::Buf<uint8_t> scratch;  // the chip form's per-window arrays (freed by dk_tcp_ctx_destroy)
};

// dk_tcp_ack_emit's own turn counter and scratch (freed by dk_tcp_ctx_destroy): it and dk_tcp_ack_process may both
// follow one dk_tcp_rx_process call, in either order.
struct dk_tcp_emit_state {
    int form = -1;       // dk_diag_tcp_ack_emit_set_form: 0 lane, 1 wave, -1 the rule
    int last_form = -1;  // the form the last dk_tcp_ack_emit call ran
    uint32_t done = 0;   // the dk_tcp_rx_process call number the last dk_tcp_ack_emit call consumed
    dk::ctl::Buf<uint8_t> scratch;
};

// dk_tcp_cc_ack's turn counter (tcp_cc_kernels.hip): it follows a dk_tcp_rx_process call as the two above do, once, and
// before that call's dk_tcp_ack_process.
struct dk_tcp_cc_state {
    uint32_t done = 0;   // the dk_tcp_rx_process call number the last dk_tcp_cc_ack call consumed
};

struct dk_tcp_order {
    int device;
    // connection c's walked segments are the frames svals[range[2c] .. range[2c + 1]), in arrival order (the segments
    // the key kernel classified, which never reach process_ack, follow up to range[2c + 2]); rec[i] = {seq, ack, meta,
    // payload} of frame i
    const uint32_t* svals;
    const uint32_t* range;
    const uint4* rec;
    bool live;              // the last dk_tcp_rx_process call completed its launches: the three arrays are its
    uint32_t n, nconns;     // that call's
    uint32_t call;          // its number on this context (from 1)
    dk::ctl::CallOrder* serial;  // the context's call order (tcp_kernels.hip, struct dk_tcp_ctx)
    dk_tcp_ack_state* ack;
    dk_tcp_emit_state* emit;
    dk_tcp_cc_state* cc;
};

// 0, or EINVAL for a null context.
int dk_tcp_ctx_order(dk_tcp_ctx* ctx, dk_tcp_order* out);

// dk_tcp_tx_commit's state in a dk_tcp_tx_ctx (tcp_commit_kernels.hip): its turn after a dk_tcp_tx_segment call, the
// form override and the chip form's per-connection bases (device; freed by dk_tcp_tx_ctx_destroy).
struct dk_tcp_commit_state {
    int form = -1;           // dk_diag_tcp_commit_set_form: 0 conn, 1 chip, -1 the rule
    int last_form = -1;      // the form the last dk_tcp_tx_commit call ran
    uint32_t seg_call = 0;   // the dk_tcp_tx_segment calls of this context that returned 0
    uint32_t seg_nbufs = 0;  // the last one's nbufs
    uint32_t done = 0;       // the dk_tcp_tx_segment call number the last dk_tcp_tx_commit call consumed
    dk::ctl::Buf<uint2> scratch;
};

// The call order of a dk_tcp_tx_ctx (tcp_tx_kernels.hip), for the calls on it that live in other files
// (dk_tcp_timers, dk_tcp_cc_send: tcp_cc_kernels.hip; dk_tcp_tx_commit, dk_tcp_rtx_piggyback: tcp_commit_kernels.hip).
// Only dk_tcp_tx_commit uses scratch of the context, its own.
struct dk_tcp_tx_ctx;
struct dk_tcp_tx_serial {
    int device;
    dk::ctl::CallOrder* serial;
    uint32_t cus;
    dk_tcp_commit_state* commit;
};

// 0, or EINVAL for a null context.
int dk_tcp_tx_ctx_serial(dk_tcp_tx_ctx* ctx, dk_tcp_tx_serial* out);

#endif  // DK_TCP_ORDER_H
