/*
 * xdrgpu.h — C ABI of the MI355X-native batched XDR (RFC 4506) marshal engine.
 *
 * This is the drop-in boundary for xdrpp's encode/decode hot path.  Every
 * entry point below replaces one reference interface; the reference
 * file:line it stands in for is cited next to it (paths relative to the
 * xdrpp source tree):
 *
 *   xdrg_plan_create      <- the compile-time field walk xdr_traits<T>::save/load
 *                            performs (xdrc/gen_hh.cc:212-250 structs,
 *                            :575-675 unions; xdrpp/types.h:676-730)
 *   xdrg_encode           <- xdr_to_opaque(r0, ..., rN-1)   xdrpp/marshal.h:264-272
 *                            (xdr_generic_put, xdrpp/marshal.h:84-137)
 *   xdrg_encode_sizes /   <- its two halves: xdr_argpack_size, then the put
 *   xdrg_encode_sized        xdrpp/marshal.h:223-234, :264-272
 *   xdrg_decode           <- xdr_from_opaque(bytes, r...)    xdrpp/marshal.h:299-306
 *                            (xdr_generic_get, xdrpp/marshal.h:142-211)
 *   xdrg_encode_msgs      <- xdr_to_msg(r) per record       xdrpp/marshal.h:252-260
 *                            (record mark: message_t::alloc, xdrpp/marshal.cc:15-31)
 *   xdrg_decode_msgs      <- xdr_from_msg(m, r) per message  xdrpp/marshal.h:278-284
 *   xdrg_index_records    <- the record boundaries of xdr_from_opaque's walk
 *                                                            xdrpp/marshal.h:299-306
 *   xdrg_index_msgs       <- the record-mark framing of read_message /
 *                            msg_sock::input                 xdrpp/srpc.cc:29-55,
 *                                                            xdrpp/msgsock.cc:38-119
 *   xdrg_serial_sizes     <- xdr_argpack_size / xdr_size     xdrpp/marshal.h:223-234,
 *                                                            xdrpp/types.h:240-244
 *   xdrg_record_depths    <- check_xdr_depth / depth_checker xdrpp/depth_checker.h:10-79
 *   xdrg_swap32/xdrg_swap64 <- swap32 / swap64               xdrpp/endian.h:56-68
 *   xdrg_rpc_dispatch     <- rpc_server_base::dispatch header decode + routing
 *                            xdrpp/server.cc:78-117, srpc.h:121-128
 *   xdrg_rpc_check_replies <- check_call_hdr + xid test      xdrpp/rpc_msg.cc:115-131,
 *                                                            xdrpp/srpc.h:61-66
 *   xdrg_rpc_replies      <- rpc_*_msg error replies         xdrpp/server.cc:8-67
 *   xdrg_rpc_verify_args  <- decode_arg per call             xdrpp/server.h:205-214,
 *                                                            srpc.h:130-134
 *   xdrg_rpc_match_replies <- rpc_sock::recv_msg: xid -> pending call
 *                                                            xdrpp/msgsock.cc:202-232
 *   xdrg_rpc_call_stats   <- rpc_call_stat(hdr), the call_result of invoke's callback
 *                                                            xdrpp/rpc_msg.cc:69-90,
 *                                                            exception.h:28-51, arpc.h:60-61
 *   xdrg_rpc_pending_retire <- recv_msg's calls_.erase, abort_all_calls
 *   (+ _workspace_size)                                      xdrpp/msgsock.cc:217-219,:190-200
 *   xdrg_rpc_verify_results <- the reply callback of asynchronous_client_base::invoke
 *                                                            xdrpp/arpc.h:59-90
 *   xdrg_rpc_reply_batch  <- srpc_service::dispatch's reply, srpc.h:130-153; the
 *   (+ _workspace_size)      order srpc_server::run writes them in, srpc.cc:83-88
 *   xdrg_rpc_next_xids    <- rpc_sock::get_xid               xdrpp/msgsock.h:118-122
 *   xdrg_rpc_call_batch   <- xdr_to_msg(hdr, args...) of asynchronous_client_base::invoke
 *   (+ _workspace_size)                                      xdrpp/arpc.h:41-59
 *   xdrg_rpc_pending_add  <- rpc_sock::send_call: calls_     xdrpp/msgsock.cc:227-232
 *   xdrg_error_message   <- the what() strings of the exception types
 *                            xdrpp/types.h:57-99, marshal.h:104-108,152-170,
 *                            :131-136,:207-210, marshal.cc:43-57
 *
 * Conventions
 *  - All data pointers passed to encode/decode are DEVICE pointers
 *    (hipMalloc / torch CUDA tensors).  No allocation happens inside the
 *    encode/decode calls; scratch comes from a caller-provided workspace.
 *  - Calls are stream-ordered and asynchronous.  Errors found by the
 *    kernels are recorded in a device-resident xdrg_status that the caller
 *    reads back with xdrg_status_read (which synchronises the stream).
 *  - No C++ exceptions cross this boundary.  Return values are
 *    XDRG_OK or a negative XDRG_E* API error; data errors are positive
 *    XDRG_ERR_* codes reported through xdrg_status.
 *  - "Native" records are the in-memory representation the kernels read
 *    (encode) or write (decode): for fixed-size schemas this is exactly the
 *    C++ struct produced by xdrc; variable-length bytes fields are staged as
 *    an xdrg_bytes_ref into a byte heap (std::vector / std::string storage is
 *    not device addressable).  See DESIGN.md "Data layout in HBM".
 */
#ifndef XDRGPU_H_INCLUDED
#define XDRGPU_H_INCLUDED 1

#ifdef __HIPCC_RTC__ /* plan-specialized kernels compiled by hiprtc */
#include <stdint.h>
#else
#include <stddef.h>
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define XDRG_ABI_VERSION 10 /* 10: xdrg_rpc_match_replies, xdrg_rpc_verify_results, xdrg_rpc_gather_results;
                                   (additive, still 10) xdrg_rpc_reply_batch, xdrg_rpc_reply_batch_workspace_size;
                                   (additive, still 10) xdrg_rpc_next_xids, xdrg_rpc_call_batch,
                                   xdrg_rpc_call_batch_workspace_size, xdrg_rpc_pending_add;
                                   (additive, still 10) xdrg_rpc_call_stats, xdrg_rpc_pending_retire,
                                   xdrg_rpc_pending_retire_workspace_size;
                                   (additive, still 10) xdrg_plan_set_compare_classes, xdrg_compare;
                                   (additive, still 10) xdrg_sort_workspace_size, xdrg_sort;
                               9: xdrg_verify, xdrg_rpc_verify_args, xdrg_rpc_gather_args */

/* ---------------------------------------------------------------------- */
/* Plan ops: a flat, wire-ordered walk of xdr_traits<T>::save.             */
/* ---------------------------------------------------------------------- */

enum xdrg_op_kind {
  XDRG_OP_U32 = 1,       /* int / unsigned / float: 4-byte native, 4-byte wire   (types.h:286-332) */
  XDRG_OP_U64 = 2,       /* hyper / unsigned hyper / double                     (types.h:286-332) */
  XDRG_OP_BOOL = 3,      /* 1-byte native bool, wire u32 0/1; any nonzero decodes true (types.h:335-349) */
  XDRG_OP_ENUM = 4,      /* int32 native; arg0/arg1 = enum value list in table (gen_hh.cc:271-305) */
  XDRG_OP_OPAQUE = 5,    /* opaque[arg0]: fixed bytes, wire pad4(arg0)          (types.h:455-470) */
  XDRG_OP_VAROPAQUE = 6, /* opaque<arg0>: native xdrg_bytes_ref                 (types.h:515-524) */
  XDRG_OP_STRING = 7,    /* string<arg0>: native xdrg_bytes_ref                 (types.h:530-587) */
  XDRG_OP_UNION = 8,     /* discriminant int32 at noff, then the selected arm   (gen_hh.cc:639-673) */
  XDRG_OP_JUMP = 9,      /* pc = arg0 (end of a union arm)                      */
  XDRG_OP_END = 10,      /* end of record                                       */
  XDRG_OP_VECTOR = 11    /* xvector<T,arg0> / pointer<T> (F_POINTER, arg0 = 1):  (types.h:365-414,476-512,591-665)
                          * native xdrg_bytes_ref {heap offset, count} of an
                          * element array with stride arg1; wire u32 count then
                          * the elements.  Fixed-size elements: the element's
                          * ops follow inline, ops [pc+1, pc+1+arg2).  Any
                          * element (F_SUB): the element is a subroutine, ops
                          * from pc arg4 to the next END, walked once per
                          * element (arg2 = 0); it may be the plan's own
                          * record (recursive types). */
};

enum xdrg_op_flags {
  XDRG_F_VALIDATE = 1,   /* ENUM / UNION: opt-in xdr_validate_enum (types.h:157-173) */
  XDRG_F_DEFAULT = 2,    /* UNION: has a default arm; arg4 = its pc             */
  XDRG_F_POINTER = 4,    /* VECTOR: xdr::pointer (count 0 or 1)                 */
  XDRG_F_SUB = 8         /* VECTOR: element subroutine at pc arg4 (below)       */
};

/*
 * One plan op (32 bytes).  `depth` is the number of class/container levels
 * (xdr_generic_put/get operator() for is_class||is_container,
 * marshal.h:129-136 and :198-205) enclosing the op, the top-level record
 * counting as 1; a union op counts its own level.  The kernels raise the
 * stack-overflow error when depth > stack_limit, which is what
 * marshaling_stack_limit (marshal.h:21,34) does in the reference.
 *
 *   kind       arg0              arg1          arg2             arg3     arg4
 *   U32/U64/BOOL  -              -             -                -        -
 *   ENUM       table idx         count         -                -        -
 *   OPAQUE     length            -             -                -        -
 *   VAROPAQUE  max length        -             -                -        -
 *   STRING     max length        -             -                -        -
 *   UNION      enum table idx    enum count    case table idx   ncases   default pc
 *   JUMP       target pc         -             -                -        -
 *
 *   VECTOR     max count         elem stride   inline ops       -        F_SUB: body pc
 *
 * The case table is a run of (int32 value, uint32 target pc) pairs in the
 * shared uint32 table.  `name` is an opaque caller id (for messages).
 *
 * Element subroutines (F_SUB).  The record's ops end with END; subroutine
 * bodies follow it, each ending with its own END.  A body's field offsets
 * are relative to the element and its depths relative to the VECTOR op:
 * an op of a body entered from a VECTOR op at (absolute) depth d sits at
 * depth d + op.depth, so an element struct's fields are at d + 1 exactly
 * as if the element were written inline.  A body may be entered from
 * itself (test_recursive, tests/xdrtest.x:29-33; rpcbind's rp__list,
 * xdrpp/rpcb_prot.x:34).  Nesting is bounded by the data and by
 * marshaling_stack_limit only: a walk keeps XDRG_SUB_FRAMES element frames
 * in registers, and records nested deeper are walked again by deep passes
 * whose frames live in the caller's workspace
 * (xdrg_deep_workspace_size: about 218 MiB + 12 bytes per record for a plan
 * that can nest that deep, 0 for any other).  A record that needs more than XDRG_MAX_FRAMES nested element
 * frames raises the stack-overflow error at the VECTOR op that would open
 * the next one; the reference's own recursion ends far earlier, in a
 * segmentation fault of its 8 MiB call stack.  A decode that fails inside
 * elements leaves rsv = 1 + the failing element's index in every container
 * on the way to the failure (0 in the others).
 */
#define XDRG_SUB_FRAMES 8
/* Element frames the record index's parse follows (xdrg_index_records);
 * a record nested deeper is XDRG_ERR_INDEX_LONG, as one past the window. */
#define XDRG_INDEX_FRAMES 16
#define XDRG_MAX_FRAMES (1u << 19)
typedef struct xdrg_op {
  uint8_t kind;
  uint8_t flags;
  uint16_t depth;
  uint32_t noff; /* byte offset of the field in the native record */
  uint32_t arg0;
  uint32_t arg1;
  uint32_t arg2;
  uint32_t arg3;
  uint32_t arg4;
  uint32_t name;
} xdrg_op;

/* Staged representation of a variable-length opaque<>/string<> field. */
typedef struct xdrg_bytes_ref {
  uint64_t off; /* byte offset into the heap buffer */
  uint32_t len; /* number of payload bytes          */
  uint32_t rsv; /* must be zero                      */
} xdrg_bytes_ref;

typedef struct xdrg_plan xdrg_plan;

enum xdrg_path {
  XDRG_PATH_FIXED_REG = 1, /* fixed size, identity layout: register permute kernel */
  XDRG_PATH_FIXED_LDS = 2, /* fixed size, general layout: LDS-staged gather kernel */
  XDRG_PATH_VAR = 3        /* variable length / unions: size pass + scan + interpreter */
};

typedef struct xdrg_plan_info {
  uint32_t path;          /* enum xdrg_path */
  uint32_t native_stride; /* bytes per native record */
  uint32_t fixed_size;    /* wire bytes per record if fixed, else 0 */
  uint32_t max_depth;     /* deepest op depth */
  uint32_t nops;
  uint32_t has_checks;    /* decode validates something (pads, enums) */
  uint64_t max_record_bytes; /* largest wire record the plan's bounds allow
                              * (fixed: fixed_size); a message's body bound */
  uint32_t group_records;    /* FIXED_LDS plans run by the group kernel: records
                              * per group (0: the LDS kernel, or not fixed) */
  uint32_t specialized;      /* var plans: 1 when the plan's specialized kernels
                              * are built (xdrg_plan_build_kernels) */
} xdrg_plan_info;

/* ---------------------------------------------------------------------- */
/* Status / errors                                                         */
/* ---------------------------------------------------------------------- */

/* API errors (return values). */
#define XDRG_OK 0
#define XDRG_EINVAL (-1)
#define XDRG_EALIGN (-2)
#define XDRG_EUNSUPPORTED (-3)
#define XDRG_EHIP (-4)
#define XDRG_ENOMEM (-5)
#define XDRG_ESPACE (-6) /* workspace or output buffer too small */

/* Data errors (reported through xdrg_status); each maps to one reference
 * exception class and what() string, see xdrg_error_message. */
enum xdrg_err {
  XDRG_ERR_NONE = 0,
  XDRG_ERR_OVERFLOW_GET = 1,    /* xdr_overflow        marshal.h:166-170 */
  XDRG_ERR_OVERFLOW_PUT = 2,    /* xdr_overflow        marshal.h:104-108 */
  XDRG_ERR_XVECTOR_BOUND = 3,   /* xdr_overflow        types.h:486-489   */
  XDRG_ERR_XSTRING_BOUND = 4,   /* xdr_overflow        types.h:539-542   */
  XDRG_ERR_NONZERO_PAD = 5,     /* xdr_should_be_zero  marshal.cc:52-55  */
  XDRG_ERR_BAD_DISCRIMINANT = 6,/* xdr_bad_discriminant gen_hh.cc:479-481,645,658 */
  XDRG_ERR_INVALID_ENUM = 7,    /* xdr_invariant_failed types.h:168-170  */
  XDRG_ERR_STACK_PUT = 8,       /* xdr_stack_overflow  marshal.h:131-132 */
  XDRG_ERR_STACK_GET = 9,       /* xdr_stack_overflow  marshal.h:200-201 */
  XDRG_ERR_SIZE_NOT_MULT4 = 10, /* xdr_bad_message_size marshal.h:157-159 */
  XDRG_ERR_TRAILING = 11,       /* xdr_bad_message_size marshal.h:207-210 */
  XDRG_ERR_POINTER_BOUND = 12,  /* xdr_overflow        types.h:605-608   */
  /* Record-marked message framing (RFC 5531 record marks of message_t). */
  XDRG_ERR_MSG_EOF = 13,        /* xdr_bad_message_size srpc.cc:36-37,51-52 */
  XDRG_ERR_MSG_SIZE4 = 14,      /* xdr_bad_message_size srpc.cc:38-39    */
  XDRG_ERR_MSG_FRAGMENT = 15,   /* xdr_bad_message_size srpc.cc:42-45    */
  XDRG_ERR_MSG_TOO_LONG = 16,   /* msg_sock maxmsglen_  msgsock.cc:99-111 */
  XDRG_ERR_MSG_MISMATCH = 17,   /* mark disagrees with the record index  */
  XDRG_ERR_MSG_COUNT = 18,      /* more messages than the index can hold */
  XDRG_ERR_LOOKBACK = 19,      /* internal: a block of the one-pass encode waited
                                   too long for the byte total of the blocks before
                                   it (never expected; the output is not written) */
  XDRG_ERR_INDEX_LONG = 20      /* xdrg_index_records: a record longer than its bound;
                                   xdrg_verify: a record nested past XDRG_INDEX_FRAMES */
};

/* Exception class a data error maps to (for host-side rethrow). */
enum xdrg_exc {
  XDRG_EXC_NONE = 0,
  XDRG_EXC_OVERFLOW = 1,          /* xdr::xdr_overflow */
  XDRG_EXC_STACK_OVERFLOW = 2,    /* xdr::xdr_stack_overflow */
  XDRG_EXC_BAD_MESSAGE_SIZE = 3,  /* xdr::xdr_bad_message_size */
  XDRG_EXC_BAD_DISCRIMINANT = 4,  /* xdr::xdr_bad_discriminant */
  XDRG_EXC_SHOULD_BE_ZERO = 5,    /* xdr::xdr_should_be_zero */
  XDRG_EXC_INVARIANT_FAILED = 6   /* xdr::xdr_invariant_failed */
};

/*
 * Device-resident status block.  first_error packs the lowest failing
 * (record, op) pair: (record << 24) | (op << 8) | code; all-ones = no error.
 * The lowest record wins because the reference stops at the first failing
 * record of the concatenated stream; within a record the lowest op index
 * wins because the reference walks fields in wire order.
 */
typedef struct xdrg_status {
  uint64_t first_error;
  uint64_t total_bytes; /* var encode: total wire bytes produced */
} xdrg_status;

typedef struct xdrg_error {
  int32_t code;     /* enum xdrg_err */
  int32_t exc;      /* enum xdrg_exc */
  uint64_t record;  /* index of the failing record */
  uint32_t op;      /* plan op index within the record (0xffffffff: record level) */
  uint32_t rsv;
  uint64_t total_bytes;
} xdrg_error;

/* ---------------------------------------------------------------------- */
/* Entry points                                                            */
/* ---------------------------------------------------------------------- */

int xdrg_abi_version(void);

/*
 * Graph capture.  Every encode, decode, size, depth, message and RPC call
 * can be captured into a hipGraph (stream capture) and replayed any number
 * of times, except xdrg_index_records' default wait for its walk's verdict
 * (a capturing stream stays asynchronous instead) and xdrg_index_msgs past
 * 16,380-byte messages.  The captured graph holds kernels only: the
 * library fills and copies device memory with kernels of its own, because
 * memset nodes of 16 bytes or more do not take effect on the replays after
 * the first under ROCm's graph packet capture (DEBUG_CLR_GRAPH_PACKET_
 * CAPTURE, on by default; tools/gpu/graph_node_probe.py, profiles/r05e),
 * which left the deep passes' list counters stale and faulted a recursive
 * plan's second replay (profiles/r04c, r05a-d).  Kernels with private
 * (scratch) memory replay correctly, also when the runtime grows its
 * scratch area between replays (profiles/r06_graph): the two interpreter
 * kernels that keep private memory (the window decode of a plan run without
 * its specialized kernels, and the encode interpreter at
 * XDRG_OPT_ENC_UNROLL 16) are capturable like the rest.  Run a plan's first
 * launch on a device outside the capture (it uploads the plan's tables).
 */

/* Validate and compile an immutable plan.  `table` holds enum value lists
 * and union case tables referenced by the ops.  native_stride is the byte
 * distance between consecutive native records.  Host-only: the plan's
 * device tables are uploaded (synchronously) to each device by its first
 * launch on that device, so run one launch per device before capturing a
 * plan's launches into a hipGraph.  A plan of 65535 or more ops is
 * XDRG_EUNSUPPORTED (status keys hold a 16-bit op index). */
int xdrg_plan_create(const xdrg_op *ops, uint32_t nops, const uint32_t *table,
                     uint32_t ntable, uint32_t native_stride, xdrg_plan **out);
void xdrg_plan_destroy(xdrg_plan *plan);
int xdrg_plan_get_info(const xdrg_plan *plan, xdrg_plan_info *info);

/* The shape of a fixed plan's encode (decode = 0) or decode program: what
 * the launcher chooses its kernel by.  Host-only, launches nothing;
 * XDRG_EUNSUPPORTED for a var plan.  With `path` of xdrg_plan_get_info:
 *   FIXED_REG and 16-byte-aligned buffers: the register kernel (has_bool and
 *     has_checks pick its instantiation, fixed_size / 16 its chunks per record);
 *   otherwise, 16-byte-aligned buffers and no checks:
 *     XDRG_OPT_FIXED_PATH 0, in_words and out_words <= 16, max_terms <= 2:
 *       the tile kernel;
 *     else XDRG_OPT_FIXED_PATH != 2, grp_G != 0 and n >= grp_G: the group
 *       kernel (grp_KT terms per word) over the whole groups of grp_G
 *       records, the LDS kernel over the n % grp_G records left;
 *   everything else: the LDS kernel, which stages whole records and their
 *     program in LDS: 4 * (in_words + 4) + 4 * roundup4(out_words) + 8 * nterms
 *     bytes for one record, nterms at least the nonzero output words.  A plan
 *     whose request exceeds the device's LDS per workgroup (160 KiB on
 *     MI355X: records past about 40 KB) gets XDRG_EUNSUPPORTED from
 *     xdrg_encode / xdrg_decode, and nothing is launched. */
typedef struct xdrg_fixed_shape {
  uint32_t in_words;   /* 4-byte words per input record  */
  uint32_t out_words;  /* 4-byte words per output record */
  uint32_t max_terms;  /* most terms (8-byte input windows or bools) of one output word */
  uint32_t has_bool;   /* the program has bool terms */
  uint32_t has_checks; /* decode program of a plan that validates pads or enums */
  uint32_t grp_G;      /* group kernel: records per group (0: no group program) */
  uint32_t grp_C;      /*   16-byte output chunks per group */
  uint32_t grp_KT;     /*   terms per output word: 1, 2 or 4 */
} xdrg_fixed_shape;
int xdrg_plan_fixed_shape(const xdrg_plan *plan, int decode, xdrg_fixed_shape *out);

/* Launch options of one plan (no reference counterpart: kernel choices and
 * launch shapes, for tests and tuning).  Every option defaults to the
 * automatic choice.  Options belong to the plan, not to the process; set
 * them before the plan is shared between threads.  Returns XDRG_EINVAL for
 * an unknown option or value. */
enum xdrg_plan_option {
  XDRG_OPT_VAR_ENCODE_KERNEL = 1, /* 0 auto, 1 per-lane walk, 3 chunk-map image   */
  XDRG_OPT_VAR_DECODE_KERNEL = 2, /* 0 auto, 1 per-lane walk, 2 LDS window         */
  XDRG_OPT_FIXED_PATH = 3,        /* non-identity layouts: 0 auto (tile kernel),
                                     2 LDS term kernel, 3 group kernel            */
  XDRG_OPT_IMAGE_BYTES = 4,       /* var encode LDS image per wave, -1 auto        */
  XDRG_OPT_WINDOW_BYTES = 5,      /* var decode LDS window per wave, -1 auto       */
  XDRG_OPT_ENC_UNROLL = 6,        /* payload chunks in flight per lane: 4, 8, 16   */
  XDRG_OPT_DEC_READAHEAD = 7,     /* window decode 32-byte read-ahead: 0 / 1       */
  XDRG_OPT_SIZE_LINEAR = 8,       /* walk-free size pass for linear plans: 0 / 1;
                                     -1 (default) only without generated kernels */
  XDRG_OPT_GRP_UNROLL = 9,        /* fixed group kernel chunks in flight, 0 auto   */
  XDRG_OPT_GRP_BLOCKS = 10,       /* fixed group kernel workgroups, 0 auto         */
  XDRG_OPT_GRP_NONTEMPORAL = 11,  /* fixed group kernel non-temporal stores: 0 / 1 */
  XDRG_OPT_SPECIALIZE = 12,       /* var plans: 1 (default) run the plan-specialized
                                     kernels (built by the first launch, or
                                     xdrg_plan_build_kernels); 0 the interpreter */
  XDRG_OPT_STAGE_BYTES = 14,     /* window decode, plans with fixed-element
                                     containers: LDS stage of a 64-record group's
                                     element arrays (written out as whole lines
                                     after the walk), -1 auto, 0 none           */
  XDRG_OPT_ENC_STREAM = 15,      /* plan-specialized word-list plans: -1 (default)
                                     the size pass + scan + a record kernel that
                                     walks each record once, first; 1 the same
                                     record kernel with no size pass and no scan
                                     (xdrg_encode: each wave's base by a look-back
                                     over the byte totals of the waves before it);
                                     0 the record kernel that walks per window   */
  XDRG_OPT_FIXED_STREAM = 16,    /* identity fixed plans (k_fixed_reg) launch
                                     shape: -1 (default) by working set (in+out
                                     up to 256 MiB: plain loads and stores, 1024
                                     workgroups; up to 1 GiB: non-temporal, 1024
                                     workgroups; beyond: non-temporal, one chunk
                                     per lane over a one-shot grid); 0 plain 1024;
                                     1 non-temporal one-shot; 2 plain one-shot;
                                     3 non-temporal 1024                         */
  XDRG_OPT_INDEX_FAST = 13        /* xdrg_index_records: 1 (default) the speculative
                                     chain walk first, then the call waits for its
                                     verdict and runs the list ranking only when a
                                     check failed; 2 the same without the wait (the
                                     list ranking is queued and skips itself: the
                                     call stays asynchronous); 0 the list ranking
                                     alone.  Same offsets, count and errors.
                                     3 (a tuning aid) the walk alone, waited for:
                                     when a check fails nothing else runs, the
                                     offsets are left as they were and the
                                     workspace keeps the walk's segment records */
};
int xdrg_plan_set_option(xdrg_plan *plan, int option, int64_t value);

/* ---------------------------------------------------------------------- */
/* Plan-specialized kernels (var plans)                                    */
/* ---------------------------------------------------------------------- */
/*
 * The generation-time form of xdr_traits<T>::save/load (xdrc/gen_hh.cc:
 * 212-250, :575-675): a plan's walk emitted as straight-line HIP source --
 * every field's checks, swaps and bytes, unions as switch statements,
 * containers as loops -- over the library's var kernels, compiled for
 * gfx950; also the plan's record-start parse for xdrg_index_records.  No
 * reference interface corresponds one to one: this is the back end xdrc
 * would run beside gen_hh.
 *
 *   xdrg_plan_kernel_source  the plan's source (NUL-terminated into buf when
 *                            cap > 0; *len = its length).  XDRG_EUNSUPPORTED
 *                            for fixed plans (their kernels are generic).
 *   xdrg_plan_build_kernels  compile now: from the kernel cache (files named
 *                            by a hash of the source under $XDRG_KERNEL_CACHE,
 *                            default kernel_cache/ beside libxdrgpu.so) or
 *                            with hiprtc.  The first var launch does this on
 *                            its own; XDRG_EHIP carries the compile log.
 *   xdrg_plan_load_kernels   attach a code object compiled ahead of time
 *                            from xdrg_plan_kernel_source (before the plan's
 *                            first launch).
 */
int xdrg_plan_kernel_source(const xdrg_plan *plan, char *buf, size_t cap, size_t *len);
int xdrg_plan_build_kernels(xdrg_plan *plan);
int xdrg_plan_load_kernels(xdrg_plan *plan, const void *code_object, size_t size);

/* Workspace bytes encode (var plans) and encode_msgs (any plan) need for n
 * records; it includes xdrg_deep_workspace_size. */
size_t xdrg_workspace_size(const xdrg_plan *plan, uint64_t n);
/* Workspace bytes decode, decode_msgs, serial_sizes and record_depths need
 * for n records: 0 except for plans whose element subroutines can nest past
 * XDRG_SUB_FRAMES, whose deep passes keep their lists of deferred records
 * and their frame slabs there, and the size walk its log of long chains
 * (about 218 MiB + 12 bytes per record; 256-byte aligned).  The memory is the caller's: no call allocates, locks or keeps
 * state between calls, so calls on different streams with different
 * workspaces run side by side, and a captured graph of them holds kernels
 * only (see "Graph capture" below). */
size_t xdrg_deep_workspace_size(const xdrg_plan *plan, uint64_t n);

/* Zero a status block (first_error = all ones) on `stream`. */
int xdrg_status_init(xdrg_status *d_status, void *stream);
/* Synchronise `stream`, then read and decode the status block. */
int xdrg_status_read(const xdrg_status *d_status, void *stream, xdrg_error *out);

/*
 * Encode n native records to the concatenated XDR stream, i.e. the bytes of
 * xdr_to_opaque(r0, ..., rn-1).
 *   d_native    n records, native_stride apart
 *   d_heap      byte heap the xdrg_bytes_ref fields point into (var plans)
 *   heap_len    heap size in bytes (reads are clamped to it)
 *   d_xdr       output; xdr_capacity bytes available
 *   d_offsets   var plans: out, n+1 uint64 record offsets (record i occupies
 *               [off[i], off[i+1]); off[n] = total).  May be NULL for fixed.
 *   stack_limit marshaling_stack_limit in effect (0xffffffff = default)
 * For a fixed plan the output is exactly n * fixed_size bytes.
 */
int xdrg_encode(const xdrg_plan *plan, const void *d_native, uint64_t n,
                const uint8_t *d_heap, uint64_t heap_len, void *d_xdr,
                uint64_t xdr_capacity, uint64_t *d_offsets,
                uint32_t stack_limit, void *d_workspace, size_t workspace_bytes,
                xdrg_status *d_status, void *stream);

/*
 * xdrg_encode (msgs = 0) or xdrg_encode_msgs (msgs = 1) in two halves, for
 * callers that size the output from the records, as xdr_to_opaque does
 * (xdr_argpack_size, then xdr_generic_put; xdrpp/marshal.h:264-272):
 *   xdrg_encode_sizes  the size pass alone (xdr_size of every record, their
 *                      scan into the workspace); the total wire bytes land
 *                      in d_status->total_bytes and size errors (a bad
 *                      discriminant) in d_status.  No output is written.
 *   xdrg_encode_sized  the encode over the sizes the first half left in the
 *                      same workspace, with the same status block (not
 *                      re-initialised), records, heap and msgs flag: the
 *                      size pass does not run again (plans whose element
 *                      subroutines nest past XDRG_SUB_FRAMES: the encode's
 *                      deep passes walk the lists of deferred records the
 *                      size pass left in the workspace).
 * Arguments as xdrg_encode / xdrg_encode_msgs; d_offsets is required by the
 * second half for every plan with msgs, for var plans without.
 */
int xdrg_encode_sizes(const xdrg_plan *plan, const void *d_native, uint64_t n,
                      const uint8_t *d_heap, uint64_t heap_len, uint32_t stack_limit, int msgs,
                      void *d_workspace, size_t workspace_bytes, xdrg_status *d_status, void *stream);
int xdrg_encode_sized(const xdrg_plan *plan, const void *d_native, uint64_t n,
                      const uint8_t *d_heap, uint64_t heap_len, void *d_out, uint64_t out_capacity,
                      uint64_t *d_offsets, uint32_t stack_limit, int msgs, void *d_workspace,
                      size_t workspace_bytes, xdrg_status *d_status, void *stream);

/*
 * Decode n records from an XDR stream of xdr_len bytes.
 * Fixed plans: the stream is n * fixed_size bytes (the records' offsets are
 *   implied); a shorter stream fails the record it runs out in
 *   (xdr_overflow), a longer one fails with "did not consume whole message",
 *   exactly as xdr_from_opaque(bytes, r0, ..., rn-1) would.
 * Var plans: d_offsets (n+1 entries, from the encoder or from RPC record
 *   framing) is required; record i is decoded from [off[i], off[i+1]) with
 *   the semantics of xdr_from_opaque on that slice.  The decoded heap is
 *   the stream itself: d_heap_out (at least xdr_len bytes) receives the
 *   stream bytes verbatim, and every decoded xdrg_bytes_ref holds the stream
 *   offset of its payload (so payloads are never gathered one by one).
 *   Passing d_heap_out == d_xdr decodes without copying: the refs then
 *   point into the input stream, which must outlive the decoded records.
 * Workspace: xdrg_deep_workspace_size(plan, n) bytes (NULL/0 for plans
 * that need none).
 */
int xdrg_decode(const xdrg_plan *plan, const void *d_xdr, uint64_t xdr_len,
                const uint64_t *d_offsets, uint64_t n, void *d_native,
                uint8_t *d_heap_out, uint64_t heap_capacity,
                uint32_t stack_limit, void *d_workspace, size_t workspace_bytes,
                xdrg_status *d_status, void *stream);

/* Heap capacity xdrg_decode needs for a stream of xdr_len bytes: xdr_len,
 * plus, for plans with xvector<T>/pointer<T> fields, an area for the
 * decoded element arrays, F * xdr_len bytes from byte align16(xdr_len),
 * every array 8-byte aligned.  F = 1 + the largest native/wire size ratio
 * of an element type.  Plans whose containers all hold fixed-size elements
 * pack the arrays of each group of 64 records (records 64g .. 64g+63) back
 * to back from align8(align16(xdr_len) + F * off[64g]), record by record
 * (a record's share is what its counts ask for, each array rounded up to
 * 8 bytes), so the arrays leave as whole cache lines; F carries 2 more for
 * that rounding.  Plans with element subroutines place record i's arrays
 * from align16(xdr_len) + F * off[i] (F: the subroutine bound, + 2).  Only
 * the xdrg_bytes_ref offsets say where an array is. */
uint64_t xdrg_decode_heap_size(const xdrg_plan *plan, uint64_t xdr_len);

/* ---------------------------------------------------------------------- */
/* Record-marked batches: message_t buffers (RFC 5531 record marking)      */
/* ---------------------------------------------------------------------- */
/*
 * A message is a 4-byte record mark BE(size | 0x80000000) followed by
 * `size` bytes: message_t's raw_data()/raw_size() (xdrpp/message.h:33-64,
 * mark written by message_t::alloc, xdrpp/marshal.cc:15-31).  A batch is
 * messages back to back, which is what msg_sock::output writes for a queue
 * of messages (xdrpp/msgsock.cc:158-188) and what read_message /
 * msg_sock::input read (xdrpp/srpc.cc:29-55, msgsock.cc:38-119).
 */
#define XDRG_MARK_LAST 0x80000000u
/* Longest message one list-ranking window of the stream indexes holds (a
 * 16 KiB segment); xdrg_index_records' record bound. */
#define XDRG_INDEX_MAX_MSG 16380u
/* Longest message a record mark can state (31 size bits). */
#define XDRG_MAX_MSG 0x7fffffffu

/*
 * Encode n records as n messages: message i = xdr_to_msg(r_i)
 * (xdrpp/marshal.h:252-260).  Arguments as xdrg_encode; d_offsets is
 * required for every plan: d_offsets[i] = byte offset of message i's mark,
 * d_offsets[n] = total bytes.  The workspace is xdrg_workspace_size bytes.
 */
int xdrg_encode_msgs(const xdrg_plan *plan, const void *d_native, uint64_t n,
                     const uint8_t *d_heap, uint64_t heap_len, void *d_out,
                     uint64_t out_capacity, uint64_t *d_offsets, uint32_t stack_limit,
                     void *d_workspace, size_t workspace_bytes, xdrg_status *d_status,
                     void *stream);

/*
 * Decode n messages: message i occupies [d_offsets[i], d_offsets[i+1]) of
 * the stream (mark included) and decodes as xdr_from_msg(m_i, r_i)
 * (xdrpp/marshal.h:278-284).  The mark must be a last-fragment mark whose
 * size is the message's byte count (XDRG_ERR_MSG_* otherwise).  Heap
 * contract as xdrg_decode (refs are stream offsets); for plans without
 * opaque<>/string<>/xvector fields d_heap_out may be NULL.
 */
int xdrg_decode_msgs(const xdrg_plan *plan, const void *d_stream, uint64_t len,
                     const uint64_t *d_offsets, uint64_t n, void *d_native,
                     uint8_t *d_heap_out, uint64_t heap_capacity, uint32_t stack_limit,
                     void *d_workspace, size_t workspace_bytes, xdrg_status *d_status,
                     void *stream);

/*
 * Record index of a stream of messages, computed on the device: the
 * framing of read_message (srpc.cc:29-55) applied message after message,
 * plus msg_sock's length limit (maxmsglen_, msgsock.cc:99-111).  Writes
 * d_offsets[k] = byte offset of mark k for every message k, d_offsets[count]
 * = len, and *d_count (a device u64) = count.  On a framing error at
 * message k (premature EOF, fragment bit clear, size bits, too long, size
 * not a multiple of 4) the error is reported at record k through d_status,
 * *d_count = k and d_offsets[k] = the failing mark's offset.  At most
 * max_msgs messages are indexed (d_offsets holds max_msgs + 1 entries);
 * more is XDRG_ERR_MSG_COUNT at record max_msgs.  Entries past count are
 * unspecified.  Any max_msg_len up to XDRG_MAX_MSG: msg_sock's is 1 MiB by
 * default (msgsock.h:29), read_message has none.  Up to XDRG_INDEX_MAX_MSG
 * the marks are walked speculatively as for xdrg_index_records (the call
 * waits once for the walk's verdict, except on a stream being captured)
 * and a list-ranking pass runs when a check fails (a damaged stream, more
 * than max_msgs messages); past it the messages longer than that are
 * walked mark by mark on the device between list-ranking windows over the
 * rest, and the call waits on the stream once or twice per window (every
 * byte is read about twice at most).
 * Workspace: xdrg_index_workspace_size(len, max_msg_len).  Its contents are
 * the call's own: the path flag xdrg_index_records leaves in its last 256
 * bytes is not part of this call's contract (with max_msg_len past
 * XDRG_INDEX_MAX_MSG those bytes hold the windows' continuation block, and
 * the index pass's own 256-byte tail sits just before them).
 */
int xdrg_index_msgs(const void *d_stream, uint64_t len, uint32_t max_msg_len,
                    uint64_t max_msgs, uint64_t *d_offsets, uint64_t *d_count,
                    void *d_workspace, size_t workspace_bytes, xdrg_status *d_status,
                    void *stream);
size_t xdrg_index_workspace_size(uint64_t len, uint32_t max_msg_len);

/*
 * Record index of n records of `plan` concatenated in one stream, the
 * input of xdr_from_opaque(bytes, r0, ..., rn-1) (xdrpp/marshal.h:299-306),
 * computed on the device.  First a speculative walk (streams of at least
 * 27776 bytes, four segments): each 6944-byte segment of the stream
 * guesses where the chain of records enters it, walks the chain (lengths,
 * counts and discriminants only) and every guess is checked against the
 * previous segment's exit; a few segments whose guess missed are walked
 * again from the true entry; when all hold and the chain
 * ends at len with exactly n records, that is the index.  Otherwise
 * (damaged streams, trailing or missing records, long records, or a guess
 * that missed: XDRG_OPT_INDEX_FAST = 0 forces this) every word position is
 * parsed as a possible record start and the chain of record ends from byte
 * 0 is ranked as for xdrg_index_msgs.  The first u32 of the 256 bytes
 * that end at xdrg_index_workspace_size(len, min(max_rec_len,
 * XDRG_INDEX_MAX_MSG)) -- the workspace's last 256 bytes when max_rec_len
 * <= XDRG_INDEX_MAX_MSG -- says which ran (1: the speculative walk).  By default
 * (XDRG_OPT_INDEX_FAST) the call waits on the stream once, for the walk's
 * verdict (not on a stream being captured into a graph: there it stays
 * asynchronous, as with XDRG_OPT_INDEX_FAST = 2).  Writes
 * d_offsets[0..n] for xdrg_decode: record r = [off[r], off[r+1]).  Where
 * the records stop parsing -- a bad discriminant, a length past its bound
 * or past the stream -- record k gets [off[k], len) and the rest [len, len),
 * so xdrg_decode reports the reference's error for record k; fewer than n
 * records end at len likewise, more leave off[n] < len (trailing bytes).
 * *d_count = the records the chain holds before it ends (all-ones when
 * it goes past record n).  max_rec_len <= XDRG_MAX_MSG.
 * max_rec_len <= XDRG_INDEX_MAX_MSG: a record longer than max_rec_len is
 * reported as XDRG_ERR_INDEX_LONG at its index.  Past XDRG_INDEX_MAX_MSG
 * the records have no length bound (xdr_from_opaque has none) and no
 * nesting bound but XDRG_MAX_FRAMES: with the plan's generated parse the
 * speculative walk takes the whole stream, records past its segments
 * parsed by a wave each through blocks of the stream in LDS (and a linked
 * list's plan, rpcb_prot.x's rp__list, parses its nodes in a loop); when
 * that walk misses the stream is indexed in rounds: one wave walks the
 * records longer than a window (lengths, counts and discriminants, its
 * element frames in the workspace) from where the chain stopped, then a
 * list-ranking window indexes the records after them up to the next long
 * one -- the call waits on the stream every round.  On a stream being
 * captured the rounds cannot run (they wait on the stream): the walk runs
 * alone, asynchronously, with the list ranking over records up to one
 * window behind it.  So a captured call indexes records past
 * XDRG_INDEX_MAX_MSG only where the walk runs and holds: the stream must
 * be at least 27776 bytes long (four 6944-byte segments; shorter streams
 * are not walked) and good -- n records ending at len.  A captured stream
 * shorter than 27776 bytes, or one the walk does not hold, gets the list
 * ranking's answer, which reports XDRG_ERR_INDEX_LONG at the first record
 * longer than XDRG_INDEX_MAX_MSG, where the same call outside a capture
 * indexes it (plans without the generated parse: XDRG_EUNSUPPORTED under
 * capture).  Plans whose records can be empty are
 * XDRG_EUNSUPPORTED.  Workspace: xdrg_index_workspace_size(len,
 * max_rec_len).
 */
int xdrg_index_records(const xdrg_plan *plan, const void *d_xdr, uint64_t len, uint64_t n,
                       uint32_t max_rec_len, uint64_t *d_offsets, uint64_t *d_count,
                       void *d_workspace, size_t workspace_bytes, xdrg_status *d_status,
                       void *stream);

/* ---------------------------------------------------------------------- */
/* RPC header batches (RFC 5531 rpc_msg, xdrpp/rpc_msg.x)                  */
/* ---------------------------------------------------------------------- */
/*
 * A batch of record-marked messages (indexed by xdrg_index_msgs: message k
 * = [d_offsets[k], d_offsets[k+1]), mark first) has its rpc_msg headers
 * decoded, one lane per message, into xdrg_rpc_hdr records:
 *
 *   xdrg_rpc_dispatch      <- rpc_server_base::dispatch, header decode and
 *                             routing (xdrpp/server.cc:78-117) plus the
 *                             procedure lookup of srpc_service::process /
 *                             arpc_service::process (srpc.h:121-128,
 *                             arpc.h:175-182)
 *   xdrg_rpc_check_replies <- the client side: archive(g, hdr),
 *                             check_call_hdr (rpc_msg.cc:115-131) and the
 *                             xid test of synchronous_client_base::invoke
 *                             (srpc.h:61-66)
 *   xdrg_rpc_replies       <- rpc_accepted_error_msg, rpc_prog_mismatch_msg,
 *                             rpc_auth_error_msg, rpc_rpc_mismatch_msg
 *                             (server.cc:8-67): the error replies of a batch
 *                             as record-marked messages
 *
 * Success replies are xdr_to_msg(rpc_success_hdr(xid), res) (srpc.h:152,
 * server.h:27-49), i.e. an argument pack: encode them with xdrg_encode_msgs
 * and a plan whose record is {xid, REPLY, MSG_ACCEPTED, AUTH_NONE, 0,
 * SUCCESS, res...} (the Python/C++ layers build it).
 *
 * The header is decoded exactly as xdr_get decodes rpc_msg: a short message
 * is xdr_overflow, an opaque_auth body over 400 bytes is the xvector bound,
 * nonzero padding is xdr_should_be_zero, an unknown msg_type / reply_stat /
 * reject_stat is a bad discriminant (accept_stat has a default arm).  Enum
 * fields are not range-checked (no xdr_validate_enum in rpc_msg.x).  A
 * header that fails is not an error of the call: its record carries the
 * XDRG_ERR_* code in `err` and the action says what the reference does
 * with it (drop it, or raise in the client).
 */
enum xdrg_rpc_action {          /* server side (xdrg_rpc_dispatch)             */
  XDRG_RPC_DISPATCH = 0,        /* registered procedure: args at body_off     */
  XDRG_RPC_DROP_MALFORMED = 1,  /* header did not decode: dropped, no reply   server.cc:84-89 */
  XDRG_RPC_DROP_NONCALL = 2,    /* mtype != CALL: dropped, no reply           server.cc:90-93 */
  XDRG_RPC_RPC_MISMATCH = 3,    /* rpcvers != 2 -> rpc_rpc_mismatch_msg       server.cc:95-96 */
  XDRG_RPC_PROG_UNAVAIL = 4,    /* unknown prog                               server.cc:98-100 */
  XDRG_RPC_PROG_MISMATCH = 5,   /* unknown vers: low/high = registered range  server.cc:102-107 */
  XDRG_RPC_PROC_UNAVAIL = 6,    /* call_dispatch found no such proc           srpc.h:125-127 */
  XDRG_RPC_GARBAGE_ARGS = 7,    /* the args fail: xdrg_rpc_verify_args, or the caller  srpc.h:132-134, server.cc:109-116 */
  XDRG_RPC_SYSTEM_ERR = 8,      /* set by the caller (accept_stat SYSTEM_ERR) */
  XDRG_RPC_AUTH_ERROR = 9       /* set by the caller: why in w[2]             server.cc:42-53 */
};
enum xdrg_rpc_status {          /* client side (xdrg_rpc_check_replies)        */
  XDRG_RPCR_OK = 0,             /* MSG_ACCEPTED + SUCCESS: result at body_off  */
  XDRG_RPCR_ACCEPT_STAT = 1,    /* xdr_call_error(accept_stat w[1])   rpc_msg.cc:120-122 */
  XDRG_RPCR_AUTH_STAT = 2,      /* xdr_call_error(auth_stat w[2])     rpc_msg.cc:124-125 */
  XDRG_RPCR_RPCVERS_MISMATCH = 3,/* xdr_call_error(RPCVERS_MISMATCH)  rpc_msg.cc:126 */
  XDRG_RPCR_NOT_REPLY = 4,      /* "call received when reply expected" rpc_msg.cc:117-118 */
  XDRG_RPCR_MALFORMED = 5,      /* archive(g, hdr) threw: code in err           srpc.h:62 */
  XDRG_RPCR_BAD_XID = 6,        /* "synchronous_client: unexpected xid"         srpc.h:64-65 */
  XDRG_RPCR_UNKNOWN_XID = 7,    /* "ignoring reply to unknown call" (xdrg_rpc_match_replies) msgsock.cc:212-216 */
  XDRG_RPCR_GARBAGE_RES = 8     /* the reply does not unmarshal (xdrg_rpc_verify_results): code in err
                                   arpc.h:87-89, rpc_msg.cc:89 */
};
/* w[] slots of xdrg_rpc_hdr */
#define XDRG_RPC_W_RPCVERS 0     /* CALL  */
#define XDRG_RPC_W_PROG 1
#define XDRG_RPC_W_VERS 2
#define XDRG_RPC_W_PROC 3
#define XDRG_RPC_W_CRED_FLAVOR 4
#define XDRG_RPC_W_REPLY_STAT 0  /* REPLY */
#define XDRG_RPC_W_STAT 1        /*   accept_stat (MSG_ACCEPTED) or reject_stat (MSG_DENIED) */
#define XDRG_RPC_W_WHY 2         /*   auth_stat (AUTH_ERROR) */
#define XDRG_RPC_W_VERF_FLAVOR 5 /* both */
#define XDRG_RPC_W_LOW 6         /* PROG_MISMATCH / RPC_MISMATCH mismatch_info */
#define XDRG_RPC_W_HIGH 7

typedef struct xdrg_rpc_hdr {   /* 64 bytes */
  uint32_t xid;
  uint16_t action;   /* xdrg_rpc_action or xdrg_rpc_status */
  uint8_t err;       /* XDRG_ERR_* of a malformed header, else 0.  A malformed
                        header keeps only action, err, end and, for
                        XDRG_ERR_BAD_DISCRIMINANT, the union in w[0]
                        (0 _body_t, 1 reply_body, 2 rejected_reply) */
  uint8_t mtype;     /* msg_type as decoded */
  uint32_t w[8];     /* XDRG_RPC_W_* */
  uint32_t cred_len; /* CALL: cred body bytes (body at mark + 36) */
  uint32_t verf_len; /* verf body bytes (CALL: body ends at body_off; REPLY: at mark + 24) */
  uint64_t body_off; /* stream offset after the header: args (CALL) / results (REPLY) */
  uint64_t end;      /* stream offset of the message end */
} xdrg_rpc_hdr;

/* A registered procedure (prog, vers, proc).  The table passed to
 * xdrg_rpc_dispatch lists every procedure of every registered interface,
 * sorted by (prog, vers, proc), no duplicates: the servers_ map of
 * rpc_server_base (server.h:218-219) plus each interface's call_dispatch
 * switch (xdrc/gen_hh.cc:757-774). */
typedef struct xdrg_rpc_proc {
  uint32_t prog, vers, proc;
  uint32_t flags; /* 0, or XDRG_RPC_PROC_IFACE_ONLY: (prog, vers) is registered
                     but this entry names no procedure (an interface whose
                     call_dispatch has no case) */
} xdrg_rpc_proc;
#define XDRG_RPC_PROC_IFACE_ONLY 1u
#define XDRG_RPC_MAX_PROCS 4096u

int xdrg_rpc_dispatch(const void *d_stream, uint64_t len, const uint64_t *d_offsets,
                      uint64_t n, const xdrg_rpc_proc *d_procs, uint32_t nprocs,
                      xdrg_rpc_hdr *d_hdrs, void *stream);

/* d_xids: the xid each reply must carry (NULL: no xid test). */
int xdrg_rpc_check_replies(const void *d_stream, uint64_t len, const uint64_t *d_offsets,
                           uint64_t n, const uint32_t *d_xids, xdrg_rpc_hdr *d_hdrs,
                           void *stream);

/* Error replies of a dispatched batch, in message order: for every header
 * whose action is RPC_MISMATCH / PROG_UNAVAIL / PROG_MISMATCH /
 * PROC_UNAVAIL / GARBAGE_ARGS / SYSTEM_ERR / AUTH_ERROR one record-marked
 * message (28, 36 or 24 bytes with its mark); other actions add nothing.
 * d_offsets[i] = offset of header i's reply (== d_offsets[i+1] when it has
 * none), d_offsets[n] = total, also in d_status->total_bytes.  An output
 * capacity below the total is XDRG_ERR_OVERFLOW_PUT at the first reply that
 * does not fit.  Workspace: xdrg_rpc_replies_workspace_size(n) bytes. */
int xdrg_rpc_replies(const xdrg_rpc_hdr *d_hdrs, uint64_t n, void *d_out, uint64_t out_capacity,
                     uint64_t *d_offsets, void *d_workspace, size_t workspace_bytes,
                     xdrg_status *d_status, void *stream);
size_t xdrg_rpc_replies_workspace_size(uint64_t n);

/* ---------------------------------------------------------------------- */
/* Per-record decode verdicts                                              */
/* ---------------------------------------------------------------------- */
/*
 * xdrg_decode reports the lowest failing (record, op) of a batch, as one
 * xdr_from_opaque over the concatenated stream would.  A server decodes
 * every call's arguments on their own (decode_arg, xdrpp/server.h:205-214:
 * archive(g, arg), g.done(), catch xdr_runtime_error): one bad record must
 * not hide the others.  xdrg_verify runs the decode's walk over n spans of
 * a stream with every check and no store, one verdict per span:
 *
 *   verdict: 0 = the record decodes; else (op << 8) | code, the low 24 bits
 *   xdrg_status.first_error would hold; op 0xffff = record level
 *
 * The verdict of a span is what xdrg_decode reports for that record decoded
 * alone (n = 1, offsets {begin, end}).  Span i is the byte range
 * [*(d_begin + i * span_stride / 8), *(d_end + i * span_stride / 8));
 * span_stride is a multiple of 8, at least 8.  With an offsets array,
 * d_end = d_begin + 1 and the stride is 8; with RPC headers, &hdr[0].body_off,
 * &hdr[0].end and 64.  Nothing outside [begin, end) is read.  Checks, in
 * order:
 *   end < begin or end > xdr_len      (op 0, XDRG_ERR_OVERFLOW_GET)
 *   begin not a multiple of 4         the same verdict (xdrg_decode has no
 *                                     such span: the records of a stream
 *                                     start at multiples of 4); never read
 *   (end - begin) not a multiple of 4 (0xffff, XDRG_ERR_SIZE_NOT_MULT4),
 *                                     the xdr_get constructor (marshal.h:
 *                                     157-159), fixed plans too
 *   the ops in wire order             stack budget (XDRG_ERR_STACK_GET)
 *                                     before space, then bounds, pads,
 *                                     validated enums and discriminants; an
 *                                     inline element fails at its element op
 *   bytes left after the walk         (0xffff, XDRG_ERR_TRAILING)
 * One kernel serves every plan (fixed, var, element subroutines): it
 * interprets the plan's ops.  A lane keeps XDRG_INDEX_FRAMES element frames;
 * a container that is the last field of its element and holds exactly one
 * element opens none, so a pointer chain (rp__list) is verified at any
 * length, bounded by stack_limit alone.  A record that needs more open
 * frames gets (that VECTOR op, XDRG_ERR_INDEX_LONG): not decided here --
 * decode it alone with xdrg_decode.
 * *d_bad_count (may be NULL) = the spans with a nonzero verdict, zeroed by
 * a kernel of the call and counted once per wave.  A plain launch: no
 * workspace, no status block, capturable into a graph (run the plan's first
 * launch on the device outside the capture).  Arguments are validated on
 * the host before any HIP call: a NULL plan, NULL verdicts or spans with
 * n > 0, or a bad stride is XDRG_EINVAL; n == 0 is XDRG_OK with nothing
 * launched (*d_bad_count is left as it was).
 */
int xdrg_verify(const xdrg_plan *plan, const void *d_xdr, uint64_t xdr_len,
                const uint64_t *d_begin, const uint64_t *d_end, uint32_t span_stride,
                uint64_t n, uint32_t stack_limit, uint32_t *d_verdicts,
                uint64_t *d_bad_count /* may be NULL */, void *stream);

/*
 * decode_arg for a whole dispatched batch, every procedure in one launch: a
 * header whose action is XDRG_RPC_DISPATCH and whose (w[PROG], w[VERS],
 * w[PROC]) is in `plans` has its arguments [body_off, end) verified with
 * that procedure's plan, as xdrg_verify does.  A nonzero verdict sets
 * action = XDRG_RPC_GARBAGE_ARGS and err = the code in place, so
 * xdrg_rpc_replies writes the reply (server.cc:109-116); the other calls go
 * on.  Every other header is untouched and gets verdict 0.  `plans` is a
 * HOST array sorted by (prog, vers, proc) with no duplicates, at most
 * XDRG_RPC_MAX_ARGPLANS entries: the plans' device tables travel as a
 * kernel argument (no upload per call; capturable).  More procedures: several
 * calls with disjoint tables.  nplans > XDRG_RPC_MAX_ARGPLANS, an unsorted
 * or duplicate table or a NULL plan is XDRG_EINVAL before any HIP call.
 */
typedef struct xdrg_rpc_argplan {
  uint32_t prog, vers, proc, rsv;
  const xdrg_plan *plan; /* the procedure's arg_tuple_type as one record */
} xdrg_rpc_argplan;
#define XDRG_RPC_MAX_ARGPLANS 64u
int xdrg_rpc_verify_args(const void *d_stream, uint64_t len, xdrg_rpc_hdr *d_hdrs, uint64_t n,
                         const xdrg_rpc_argplan *plans, uint32_t nplans, uint32_t stack_limit,
                         uint32_t *d_verdicts /* n, may be NULL */, void *stream);

/*
 * One procedure's arguments as an indexed stream: the headers with action
 * XDRG_RPC_DISPATCH and (w[PROG], w[VERS], w[PROC]) == (prog, vers, proc),
 * in message order.  d_index[k] = the message index of the k-th, d_offsets[k]
 * = the offset of its argument bytes in d_args, d_offsets[count] = the
 * total (also in d_status->total_bytes), *d_count = count; the bytes
 * [body_off, end) are copied verbatim, at any length, so
 * xdrg_decode(plan, d_args, total, d_offsets, count, ...) decodes them.  A
 * header with end < body_off or end > len is skipped (not selected: nothing
 * of the stream is read for it).  A capacity below the total is
 * XDRG_ERR_OVERFLOW_PUT (record = the message index, op 0xffff) at the
 * first message that does not fit; d_status is not initialised by the call
 * (xdrg_status_init).  d_offsets holds n + 1 entries, d_index n; entries
 * past count are unspecified.  Workspace:
 * xdrg_rpc_gather_workspace_size(n) bytes.
 */
int xdrg_rpc_gather_args(const void *d_stream, uint64_t len, const xdrg_rpc_hdr *d_hdrs, uint64_t n,
                         uint32_t prog, uint32_t vers, uint32_t proc,
                         uint8_t *d_args, uint64_t args_capacity,
                         uint64_t *d_offsets /* n+1 */, uint64_t *d_index /* n */, uint64_t *d_count,
                         void *d_workspace, size_t workspace_bytes, xdrg_status *d_status, void *stream);
size_t xdrg_rpc_gather_workspace_size(uint64_t n);

/* ---------------------------------------------------------------------- */
/* Asynchronous client replies                                             */
/* ---------------------------------------------------------------------- */
/*
 * xdrg_rpc_check_replies with d_xids is the synchronous client: one call
 * outstanding, replies in order (xdrpp/srpc.h:61-66).  The reference's other
 * client, asynchronous_client_base::invoke over rpc_sock (xdrpp/arpc.h:41-91,
 * xdrpp/msgsock.cc:202-232), keeps a table of outstanding calls keyed by xid
 * (rpc_sock::calls_) and takes replies in any order: it looks the xid up,
 * drops a reply to an unknown call, erases the call, decodes the header,
 * decodes the result with that call's result type, requires g.done(), and
 * turns any xdr_runtime_error into GARBAGE_RES for that call alone.  The
 * three calls below do this for a batch.
 *
 * A pending table is a device array of xdrg_rpc_call sorted by xid as
 * unsigned, ascending, no duplicates.  `res` names the call's result type:
 * an index into a host table of result plans.  An unsorted table is the
 * caller's error: matches are then unspecified, but nothing outside the
 * arrays is read or written.
 */
typedef struct xdrg_rpc_call { uint32_t xid; uint32_t res; } xdrg_rpc_call; /* 8 bytes */
#define XDRG_RPC_NO_CALL 0xffffffffffffffffull

/*
 * rpc_sock::recv_msg (msgsock.cc:202-232) for every message of a batch.
 * d_hdrs holds what xdrg_rpc_check_replies(..., d_xids = NULL, ...) wrote
 * for the same batch.  The message itself is read, not the header record (a
 * malformed header keeps no xid).  Per message, with body size
 * d_offsets[i+1] - d_offsets[i] - 4:
 *   size < 8             header untouched, d_call[i] = XDRG_RPC_NO_CALL (the
 *                        reference's abort_all_calls is a connection matter
 *                        and stays with the caller); so is a message whose
 *                        offsets are not inside the stream (never read)
 *   word 1 == CALL       header untouched (NOT_REPLY or MALFORMED), NO_CALL
 *   word 1 == REPLY      binary search of word 0 in the table:
 *     no entry           action = XDRG_RPCR_UNKNOWN_XID, NO_CALL
 *                        ("ignoring reply to unknown call", msgsock.cc:212-216)
 *     entry c            the lowest such message index i wins (the reference
 *                        erases the call at its first reply, whether or not
 *                        that reply decodes, msgsock.cc:217-219):
 *                        d_call[i] = c, d_reply_of[c] = i, and its header
 *                        keeps its action, MALFORMED included.  Every later
 *                        reply to c becomes UNKNOWN_XID with NO_CALL
 *   any other word 1     untouched, NO_CALL
 * d_reply_of[c] = XDRG_RPC_NO_CALL for a call no message answers.  The
 * outcome is a function of the inputs only: a fill, a 64-bit atomicMin of
 * the message index into d_reply_of[c], then a kernel that compares.  No
 * workspace, no status block, no memset node: capturable like xdrg_verify.
 * ncalls == 0 is legal (d_calls may be NULL; every REPLY becomes
 * UNKNOWN_XID).  n == 0 and ncalls == 0: XDRG_OK, nothing launched; n == 0
 * and ncalls > 0: d_reply_of is filled with NO_CALL.  Validated on the host
 * before any HIP call: NULL required pointers are XDRG_EINVAL, misaligned
 * ones (headers 16, u64 arrays and calls 8, stream 4) XDRG_EALIGN.
 */
int xdrg_rpc_match_replies(const void *d_stream, uint64_t len, const uint64_t *d_offsets, uint64_t n,
                           const xdrg_rpc_call *d_calls, uint64_t ncalls, xdrg_rpc_hdr *d_hdrs,
                           uint64_t *d_call /* n */, uint64_t *d_reply_of /* ncalls */, void *stream);

/*
 * The body of the reply callback of arpc.h:59-90 for every matched reply,
 * all result types in one launch.  `plans` is a HOST array of nplans <=
 * XDRG_RPC_MAX_ARGPLANS plan pointers: plans[k] serves res == res_base + k; a
 * NULL entry is a void result (xdr_void: a plan cannot be empty).  More
 * result types: several calls with disjoint ranges.  A message is handled by
 * the call whose range holds its call's res; it needs d_call[i] = c <
 * ncalls.  By its action:
 *   OK            [body_off, end) is verified exactly as xdrg_verify does
 *                 (NULL plan: the span rules, then (0xffff, XDRG_ERR_TRAILING)
 *                 when end > body_off).  A nonzero verdict sets action =
 *                 XDRG_RPCR_GARBAGE_RES and err = the code (arpc.h:87-89)
 *   ACCEPT_STAT, AUTH_STAT, RPCVERS_MISMATCH
 *                 g.done() still runs (arpc.h:67-69): end != body_off is
 *                 verdict (0xffff, XDRG_ERR_TRAILING), GARBAGE_RES, err =
 *                 XDRG_ERR_TRAILING; else the header is untouched, verdict 0
 *   MALFORMED     the header threw: GARBAGE_RES, err kept, verdict
 *                 (0xffff << 8) | err
 * Every other message is untouched, verdict 0.  The plans' device tables
 * travel as a kernel argument, as in xdrg_rpc_verify_args (capturable; run
 * each plan's first launch on the device outside the capture).  nplans >
 * XDRG_RPC_MAX_ARGPLANS or NULL required pointers with n > 0 are XDRG_EINVAL
 * before any HIP call.
 */
int xdrg_rpc_verify_results(const void *d_stream, uint64_t len, xdrg_rpc_hdr *d_hdrs,
                            const uint64_t *d_call /* n */, uint64_t n,
                            const xdrg_rpc_call *d_calls, uint64_t ncalls,
                            const xdrg_plan *const *plans /* HOST, nplans */, uint32_t nplans,
                            uint32_t res_base, uint32_t stack_limit,
                            uint32_t *d_verdicts /* n, may be NULL */, void *stream);

/*
 * One result type's bytes as an indexed stream: xdrg_rpc_gather_args with the
 * selection action == XDRG_RPCR_OK, d_call[i] = c < ncalls and
 * d_calls[c].res == res, in message order.  d_index[k] = the message index of
 * the k-th selected reply; d_results and d_offsets feed xdrg_decode.
 * Capacity, skipped headers, d_status and the sizes of d_offsets and d_index
 * are as in xdrg_rpc_gather_args.  Workspace:
 * xdrg_rpc_gather_results_workspace_size(n) bytes.
 */
int xdrg_rpc_gather_results(const void *d_stream, uint64_t len, const xdrg_rpc_hdr *d_hdrs,
                            const uint64_t *d_call /* n */, uint64_t n,
                            const xdrg_rpc_call *d_calls, uint64_t ncalls, uint32_t res,
                            uint8_t *d_results, uint64_t results_capacity,
                            uint64_t *d_offsets /* n+1 */, uint64_t *d_index /* n */, uint64_t *d_count,
                            void *d_workspace, size_t workspace_bytes, xdrg_status *d_status, void *stream);
size_t xdrg_rpc_gather_results_workspace_size(uint64_t n);

/* ---------------------------------------------------------------------- */
/* Server reply batch                                                      */
/* ---------------------------------------------------------------------- */
/*
 * srpc_server::run (xdrpp/srpc.cc:83-88) reads a message, dispatches it and
 * writes its reply before it reads the next one: the socket carries one reply
 * per answered call, in call order -- xdr_to_msg(rpc_success_hdr(xid), *res)
 * (srpc.h:152, server.h:27-49) for a call that was served, one of the
 * rpc_*_msg replies (server.cc:8-67) for a call that failed.
 * xdrg_rpc_reply_batch writes that stream for a dispatched batch whose
 * handlers have run: the results come as up to XDRG_RPC_MAX_RESULT_SRCS
 * sources, each the output of one xdrg_encode and the message every result
 * answers (xdrg_rpc_gather_args' d_index).
 *
 * Message i, in message order:
 *   action RPC_MISMATCH, PROG_UNAVAIL, PROG_MISMATCH, PROC_UNAVAIL,
 *   GARBAGE_ARGS, SYSTEM_ERR, AUTH_ERROR
 *                  exactly the bytes xdrg_rpc_replies writes for the header.
 *                  A result that names such a message is not used.
 *   DISPATCH with a winning entry
 *                  the mark BE((24 + L) | XDRG_MARK_LAST), the six words xid,
 *                  REPLY (1), MSG_ACCEPTED (0), AUTH_NONE (0), 0, SUCCESS (0)
 *                  big-endian, then the entry's L result bytes verbatim (a
 *                  void result: L = 0, 28 bytes).  The result bytes are not
 *                  validated as XDR: the server trusts its own encoder.
 *   DISPATCH with no entry (an asynchronous service that has not answered
 *   yet), DROP_*, any other action
 *                  no reply: d_offsets[i] == d_offsets[i+1].
 * Entry k of a source, k < min(*d_count, count_cap), names message
 * d_index[k] and holds the bytes [d_offsets[k], d_offsets[k+1]) of d_bytes
 * (d_offsets NULL: [k * fixed_size, (k+1) * fixed_size); d_bytes NULL: no
 * bytes, and d_offsets is not read).  An entry is not usable, and nothing of
 * d_bytes is read for it, when index >= n, when its message's action is not
 * DISPATCH, when its span has end < begin or end > bytes_len, when its offset
 * or length is not a multiple of 4, or when 24 + L > XDRG_MAX_MSG.  Of the
 * usable entries that name message i the lowest (source, position) wins: a
 * fill, a 64-bit atomicMin of the packed pair into an owner word per
 * message, then a compare, as in xdrg_rpc_match_replies -- the outcome is a
 * function of the inputs only.  *d_unused (may be NULL) = the entries that
 * produced no reply, unusable or beaten by a lower entry; written by a
 * kernel of the call (no memset, and no atomic on the one word).
 *
 * d_offsets[i] = the offset of message i's reply, d_offsets[n] = the total,
 * also in d_status->total_bytes.  A capacity below the total is
 * XDRG_ERR_OVERFLOW_PUT at the first message that does not fit (record = the
 * message index, op 0xffff); every reply before it is written as in an
 * unbounded call and nothing at or past out_capacity is written.  d_status
 * is not initialised by the call (xdrg_status_init).
 *
 * Validated on the host before any HIP call.  XDRG_EINVAL: NULL d_offsets or
 * d_status; NULL d_hdrs with n > 0; NULL srcs with nsrcs > 0; nsrcs >
 * XDRG_RPC_MAX_RESULT_SRCS; a source with count_cap > 0 and NULL d_index,
 * with d_bytes NULL and fixed_size != 0, or with d_bytes set, d_offsets NULL
 * and fixed_size zero or not a multiple of 4.  XDRG_EALIGN: headers not
 * 16-aligned, u64 arrays not 8-aligned, d_out or d_bytes not 4-aligned.
 * XDRG_ESPACE: workspace below xdrg_rpc_reply_batch_workspace_size(n).
 * n == 0: d_offsets[0] and the total are zeroed as xdrg_rpc_replies does, and
 * *d_unused = the sum of the sources' counts.
 *
 * Kernels only: no memset node, no wait on the stream, no state; capturable
 * into a graph on one stream.  `srcs` is a HOST array of device pointers:
 * the sources travel as kernel arguments, as the plans of
 * xdrg_rpc_verify_args do.
 */
typedef struct xdrg_rpc_result_src { /* 48 bytes */
  const uint8_t *d_bytes;    /* xdr_to_opaque(r0, ..., r_count-1): xdrg_encode's output.  NULL: every result is void */
  const uint64_t *d_offsets; /* count + 1 (xdrg_encode's d_offsets); NULL: result k = [k*fixed_size, (k+1)*fixed_size) */
  const uint64_t *d_index;   /* count message numbers (xdrg_rpc_gather_args' d_index); any order */
  const uint64_t *d_count;   /* device count (the gather's d_count); NULL: count_cap is the count */
  uint64_t bytes_len;        /* bytes readable at d_bytes */
  uint32_t count_cap;        /* host bound on the count (sizes the launch); min(*d_count, count_cap) entries are used */
  uint32_t fixed_size;       /* used when d_offsets is NULL (0 with d_bytes NULL) */
} xdrg_rpc_result_src;
#define XDRG_RPC_MAX_RESULT_SRCS 64u

size_t xdrg_rpc_reply_batch_workspace_size(uint64_t n);
int xdrg_rpc_reply_batch(const xdrg_rpc_hdr *d_hdrs, uint64_t n,
                         const xdrg_rpc_result_src *srcs /* HOST */, uint32_t nsrcs,
                         void *d_out, uint64_t out_capacity, uint64_t *d_offsets /* n+1 */,
                         uint64_t *d_unused /* may be NULL */,
                         void *d_workspace, size_t workspace_bytes,
                         xdrg_status *d_status, void *stream);

/* ---------------------------------------------------------------------- */
/* Client call batch                                                       */
/* ---------------------------------------------------------------------- */
/*
 * asynchronous_client_base::invoke over rpc_sock (xdrpp/arpc.h:41-59,
 * xdrpp/msgsock.h:118-122, xdrpp/msgsock.cc:227-232) takes an xid, marshals
 * xdr_to_msg(hdr, args...) and remembers the call in calls_.  The three
 * calls below do this for a batch whose calls go to many procedures: the
 * xids, the one stream xdrg_index_msgs / xdrg_rpc_dispatch read on the
 * server, and the pending table xdrg_rpc_match_replies searches.  All three
 * validate on the host before any HIP call, launch kernels only (no memset
 * node, no wait on the stream, no state; capturable on one stream) and
 * neither read nor write anything outside the given arrays, whatever these
 * hold.
 */

/*
 * rpc_sock::get_xid() n times: d_xids[k] is what the (k+1)-th get_xid()
 * returns when every earlier one was followed by send_call -- the (k+1)-th
 * value after last_xid, counting upwards mod 2^32, that is not in the pending
 * table d_calls (sorted as for xdrg_rpc_match_replies).  One lane per xid, no
 * dependence between lanes: with r(x) = (x - last_xid - 1) mod 2^32 and the
 * table read from lower_bound(last_xid + 1) on and around its end, R[0] <
 * R[1] < ... are the pending values in the order get_xid meets them, and
 * xid_k = last_xid + 1 + k + j for the smallest j with R[j] - j > k (64-bit
 * arithmetic; j = ncalls when there is none).
 *
 * One departure from the reference: its loop `while (calls_.find(++xid_) !=
 * calls_.end())` is written to stop at xid_ == 0 even when 0 is pending, and
 * would hand out a duplicate.  Here a pending 0 is skipped like any other
 * value.
 *
 * XDRG_EINVAL: ncalls + n > 0xffffffff (no n free values are left), NULL
 * d_calls with ncalls > 0, NULL d_xids with n > 0.  XDRG_EALIGN: d_calls not
 * 8-aligned, d_xids not 4-aligned.  n == 0: XDRG_OK, nothing launched.  An
 * unsorted table gives unspecified xids.
 */
int xdrg_rpc_next_xids(const xdrg_rpc_call *d_calls, uint64_t ncalls, uint32_t last_xid,
                       uint64_t n, uint32_t *d_xids /* n */, void *stream);

/*
 * The call stream.  The arguments come as up to XDRG_RPC_MAX_ARG_SRCS
 * sources, each the output of one xdrg_encode for one procedure and the call
 * position (0..n-1) every argument record belongs to.
 *
 * Call position i, in call order:
 *   with a winning entry of L argument bytes
 *                  the mark BE((40 + L) | XDRG_MARK_LAST), the ten words
 *                  d_xids[i], CALL (0), 2, prog, vers, proc, 0, 0, 0, 0
 *                  big-endian (cred and verf: AUTH_NONE opaque_auth with
 *                  empty bodies, which is all invoke sends), then the L bytes
 *                  verbatim: what xdrg_encode_msgs writes for the record
 *                  "ten header words, then the arguments".  The argument
 *                  bytes are not validated as XDR.
 *   with no entry  no message: d_offsets[i] == d_offsets[i+1].
 * d_sent[i] (may be NULL) = {d_xids[i], res of the winning source}, or
 * {d_xids[i], XDRG_RPC_RES_UNSENT} for a position without a message: the
 * d_new of xdrg_rpc_pending_add.
 *
 * Entry k of a source, k < min(*d_count, count_cap), names position
 * d_index[k] and holds the bytes [d_offsets[k], d_offsets[k+1]) of d_bytes
 * (d_offsets NULL: [k * fixed_size, (k+1) * fixed_size); d_bytes NULL: no
 * bytes, and d_offsets is not read).  An entry is not usable, and nothing of
 * d_bytes is read for it, when index >= n, when its span has end < begin or
 * end > bytes_len, when its offset or length is not a multiple of 4, or when
 * 40 + L > XDRG_MAX_MSG.  Of the usable entries that name position i the
 * lowest (source, position) wins: a fill, a 64-bit atomicMin of the packed
 * pair into an owner word per position, then a compare -- the outcome is a
 * function of the inputs only.  d_counts (may be NULL): d_counts[0] = the
 * positions without a message, d_counts[1] = the entries that produced none,
 * unusable or beaten by a lower entry; both written by a kernel of the call
 * from tile sums (no memset, and no atomic on the one word).
 *
 * d_offsets[i] = the offset of position i's message, d_offsets[n] = the
 * total, also in d_status->total_bytes.  A capacity below the total is
 * XDRG_ERR_OVERFLOW_PUT at the first position that does not fit (record = the
 * position, op 0xffff); every message before it is written as in an unbounded
 * call and nothing at or past out_capacity is written.  d_status is not
 * initialised by the call (xdrg_status_init).
 *
 * XDRG_EINVAL: NULL d_offsets or d_status; NULL d_xids with n > 0; NULL srcs
 * with nsrcs > 0; nsrcs > XDRG_RPC_MAX_ARG_SRCS; a source with count_cap > 0
 * and NULL d_index, with d_bytes NULL and fixed_size != 0, or with d_bytes
 * set, d_offsets NULL and fixed_size zero or not a multiple of 4; NULL d_out
 * with a capacity.  XDRG_EALIGN: u64 arrays, d_sent or d_counts not
 * 8-aligned, d_xids, d_out or d_bytes not 4-aligned.  XDRG_ESPACE: workspace
 * below xdrg_rpc_call_batch_workspace_size(n).  n == 0: d_offsets[0] and the
 * total are zeroed, d_counts = {0, the sum of the sources' counts}.
 *
 * `srcs` is a HOST array of device pointers: the sources travel as kernel
 * arguments, as those of xdrg_rpc_reply_batch do.
 */
typedef struct xdrg_rpc_arg_src { /* 64 bytes */
  const uint8_t *d_bytes;    /* xdrg_encode's output for this procedure's arguments.  NULL: no arguments */
  const uint64_t *d_offsets; /* count + 1 (xdrg_encode's d_offsets); NULL: entry k = [k*fixed_size, (k+1)*fixed_size) */
  const uint64_t *d_index;   /* count call positions (0..n-1); any order */
  const uint64_t *d_count;   /* device count; NULL: count_cap is the count */
  uint64_t bytes_len;        /* bytes readable at d_bytes */
  uint32_t count_cap;        /* host bound on the count (sizes the launch); min(*d_count, count_cap) entries are used */
  uint32_t fixed_size;       /* used when d_offsets is NULL (0 with d_bytes NULL) */
  uint32_t prog, vers, proc; /* P::interface_type::program / version, P::proc (arpc.h:46-48) */
  uint32_t res;              /* the procedure's result type number, for the pending table */
} xdrg_rpc_arg_src;
#define XDRG_RPC_MAX_ARG_SRCS 64u
#define XDRG_RPC_RES_UNSENT 0xffffffffu

size_t xdrg_rpc_call_batch_workspace_size(uint64_t n);
int xdrg_rpc_call_batch(const uint32_t *d_xids, uint64_t n,
                        const xdrg_rpc_arg_src *srcs /* HOST */, uint32_t nsrcs,
                        void *d_out, uint64_t out_capacity, uint64_t *d_offsets /* n+1 */,
                        xdrg_rpc_call *d_sent /* n, call order; may be NULL */,
                        uint64_t *d_counts /* 2, may be NULL */,
                        void *d_workspace, size_t workspace_bytes, xdrg_status *d_status, void *stream);

/*
 * rpc_sock::calls_ after the sends: d_merged = the sorted table d_calls
 * merged with d_new, where d_new is xdrg_rpc_call_batch's d_sent over
 * xdrg_rpc_next_xids' xids -- ascending as unsigned except for at most one
 * descent (the wrap past 2^32 - 1), and disjoint from the table.  New entry k
 * lands at lower_bound(table, xid_k) plus the new entries with a smaller
 * xid: (n - w) + k before the wrap point w, k - w from it on (w by a binary
 * search over d_new); old entry j lands at j plus the new entries below it.
 * d_old_pos[j] / d_new_pos[k] (may be NULL) = where old entry j / new entry k
 * went.
 *
 * EVERY entry of d_new is merged, XDRG_RPC_RES_UNSENT ones included: a caller
 * that leaves calls unsent filters them first.  A d_new or a table that
 * breaks the precondition gives an unspecified table, but every write stays
 * inside d_merged and the two position arrays.
 *
 * XDRG_EINVAL: NULL d_calls with ncalls > 0, NULL d_new with n > 0, NULL
 * d_merged with ncalls + n > 0; d_merged equal to or overlapping d_calls or
 * d_new.  XDRG_EALIGN: any array not 8-aligned.  ncalls + n == 0: XDRG_OK,
 * nothing launched.
 */
int xdrg_rpc_pending_add(const xdrg_rpc_call *d_calls, uint64_t ncalls,
                         const xdrg_rpc_call *d_new /* n */, uint64_t n,
                         xdrg_rpc_call *d_merged /* ncalls + n */,
                         uint64_t *d_old_pos /* ncalls, may be NULL */,
                         uint64_t *d_new_pos /* n, may be NULL */, void *stream);

/* ---------------------------------------------------------------------- */
/* Settling a reply batch                                                  */
/* ---------------------------------------------------------------------- */
/*
 * rpc_sock does three things with calls_: send_call emplaces the call
 * (xdrpp/msgsock.cc:227-232; xdrg_rpc_pending_add), recv_msg erases it at its
 * first reply, before the callback runs (msgsock.cc:217-219), and
 * abort_all_calls empties calls_ and hands every callback nullptr
 * (msgsock.cc:190-200), which invoke's lambda turns into
 * rpc_call_stat::NETWORK_ERROR (xdrpp/arpc.h:60-61).  The callback receives a
 * call_result per call, which is an rpc_call_stat (xdrpp/exception.h:28-51)
 * built by rpc_call_stat(hdr) (xdrpp/rpc_msg.cc:69-90).  The two calls below
 * give, after a reply batch, every pending call's rpc_call_stat in one device
 * array and the table that goes into the next round: calls_ as the reference
 * would hold it.  Over that table xdrg_rpc_match_replies reports a late
 * duplicate of a retired call as XDRG_RPCR_UNKNOWN_XID (msgsock.cc:212-216)
 * and xdrg_rpc_next_xids skips only what is pending now (msgsock.h:118-122).
 *
 * Both validate on the host before any HIP call, launch kernels only (no
 * memset or memcpy node, no wait on the stream, no state; capturable on one
 * stream), use no atomic -- the result is a function of the inputs only --
 * and neither read nor write anything outside the given arrays, whatever
 * these hold.
 */
typedef struct xdrg_rpc_call_stat { uint32_t type; uint32_t stat; } xdrg_rpc_call_stat; /* 8 bytes */
/* type: rpc_call_stat::stat_type in the reference's order (exception.h:29-36) */
#define XDRG_RPCS_ACCEPT_STAT 0u      /* stat = accept_stat; {0, 0} is success (operator bool, exception.h:48-50) */
#define XDRG_RPCS_AUTH_STAT 1u        /* stat = auth_stat (rj_why) */
#define XDRG_RPCS_RPCVERS_MISMATCH 2u /* stat = 0 */
#define XDRG_RPCS_GARBAGE_RES 3u      /* stat = 0 */
#define XDRG_RPCS_NETWORK_ERROR 4u    /* stat = 0 */
#define XDRG_RPCS_BAD_ALLOC 5u        /* named for completeness; never produced */
#define XDRG_RPCS_PENDING 0xffffffffu /* not a reference value: no reply yet */

/*
 * What cb receives for every pending call.  One lane per table entry c;
 * d_hdrs holds the batch's headers after xdrg_rpc_verify_results, d_reply_of
 * what xdrg_rpc_match_replies wrote.  With i = d_reply_of[c]:
 *   i == XDRG_RPC_NO_CALL  {unanswered, 0}.  unanswered is XDRG_RPCS_PENDING
 *                          (a reply batch in normal operation) or
 *                          XDRG_RPCS_NETWORK_ERROR (the caller runs
 *                          abort_all_calls: every call still outstanding
 *                          gets cb(NETWORK_ERROR))
 *   i < n                  by d_hdrs[i].action, as rpc_call_stat(hdr) and the
 *                          catch of arpc.h:87-89 give it:
 *     XDRG_RPCR_OK                {ACCEPT_STAT, 0}
 *     XDRG_RPCR_ACCEPT_STAT       {ACCEPT_STAT, w[XDRG_RPC_W_STAT]}
 *     XDRG_RPCR_AUTH_STAT         {AUTH_STAT, w[XDRG_RPC_W_WHY]}
 *     XDRG_RPCR_RPCVERS_MISMATCH  {RPCVERS_MISMATCH, 0}
 *     anything else               {GARBAGE_RES, 0}: GARBAGE_RES, MALFORMED,
 *                                 NOT_REPLY and any action a matched reply
 *                                 cannot carry
 *   any other i            (at or past n: no message of this batch)
 *                          {GARBAGE_RES, 0}; no header is read
 * XDRG_EINVAL: unanswered neither of the two values; with ncalls > 0, NULL
 * d_reply_of or d_stats, or NULL d_hdrs with n > 0.  XDRG_EALIGN: d_hdrs not
 * 16-aligned, d_reply_of or d_stats not 8-aligned.  XDRG_EUNSUPPORTED: more
 * than 0x7fffffff workgroups.  ncalls == 0: XDRG_OK, nothing launched.
 * Nothing of d_hdrs is written, and nothing of it is read for a call without
 * a reply in this batch.
 */
int xdrg_rpc_call_stats(const xdrg_rpc_hdr *d_hdrs, uint64_t n,
                        const uint64_t *d_reply_of /* ncalls, table order */, uint64_t ncalls,
                        uint32_t unanswered, xdrg_rpc_call_stat *d_stats /* ncalls */, void *stream);

/*
 * calls_ after the erases of a reply batch.  Entry j of the sorted table is
 * kept iff d_reply_of[j] == XDRG_RPC_NO_CALL; any other value means the entry
 * was answered, whatever the value is (as in xdrg_rpc_call_stats).  The kept
 * entries go to d_kept[0..count) in table order, so d_kept is again sorted
 * with no duplicates; *d_count = count; d_kept_pos[j] (may be NULL) = the new
 * table position of old entry j, or XDRG_RPC_NO_CALL when it was retired.
 * Entries of d_kept at or past count are unspecified; nothing at or past
 * d_kept + ncalls is written, and nothing of d_calls or d_reply_of is.
 *
 * An ordered stream compaction in three passes: the kept entries of every
 * 256-entry tile; the exclusive scan of the tile counts in one workgroup,
 * which also writes *d_count; a scatter in which a lane's rank is the kept
 * lanes below it in its wave's 64-bit ballot, plus the waves before it in the
 * tile, plus the tile's base.  No atomic counter (the order is the table's).
 * The workspace holds the tile counts only and need not be initialised.
 *
 * XDRG_EINVAL: NULL d_count; with ncalls > 0, NULL d_calls, d_reply_of or
 * d_kept, or d_kept equal to or overlapping d_calls (an in-place compaction
 * would race between workgroups).  XDRG_EALIGN: any array not 8-aligned.
 * XDRG_ESPACE: workspace below xdrg_rpc_pending_retire_workspace_size(ncalls).
 * XDRG_EUNSUPPORTED: more than 0x7fffffff workgroups.  ncalls == 0: *d_count =
 * 0 is still written, by a kernel; no workspace is needed.
 */
size_t xdrg_rpc_pending_retire_workspace_size(uint64_t ncalls);
int xdrg_rpc_pending_retire(const xdrg_rpc_call *d_calls, uint64_t ncalls,
                            const uint64_t *d_reply_of /* ncalls */,
                            xdrg_rpc_call *d_kept /* ncalls entries of room */,
                            uint64_t *d_kept_pos /* ncalls, may be NULL */,
                            uint64_t *d_count /* device u64 */,
                            void *d_workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------- */
/* The receive side                                                        */
/* ---------------------------------------------------------------------- */
/*
 * Every stage above starts from one device buffer of whole record-marked
 * messages.  A server or an asynchronous client has many sockets instead, each
 * of which has handed over some number of bytes that usually ends inside a
 * mark or inside a body.  xdrg_rpc_recv_batch is msg_sock::input
 * (xdrpp/msgsock.cc:38-119) for all of them in one call: a partial read is
 * kept for the next one (rdpos_, rdmsg_), every whole message is delivered
 * (rcb_), a clear fragment bit is ECONNRESET (:86-91), a size above maxmsglen_
 * is E2BIG as soon as the mark is read (:99-117), and what was delivered
 * before a failure stays delivered.  With XDRG_RECV_RPC_SOCK it also applies
 * rpc_sock::recv_msg's test (:202-225), which closes the connection at the
 * first message shorter than 8 bytes or whose word 1 is neither CALL nor REPLY
 * (rpc_tcp_listener_common::receive_cb, xdrpp/server.cc:152-158, deletes the
 * socket).  One bad connection does not hide the others.
 *
 * Input.  Connection c's bytes are d_buf[begin, begin + len); begin is a
 * multiple of 4, the segments are ascending and disjoint (begin[c] + len[c] <=
 * begin[c + 1] <= buf_len), len is arbitrary (0, 1..3, not a multiple of 4:
 * TCP delivers any count).  The table lives on the device: the kernels clamp
 * every segment into [0, buf_len) (begin rounded down to a multiple of 4) and
 * never read outside d_buf nor write outside the outputs, whatever it holds.
 *
 * Framing.  Each connection is framed on its own by the rules xdrg_index_msgs
 * follows (read_message's order of checks, xdrpp/srpc.cc:29-55, with
 * msg_sock's length rule), except that a cut tail is no error: the connection
 * stays XDRG_CONN_OPEN, consumed stops at the last whole message and need
 * says how long the tail must become.  An empty message (size 0) is
 * delivered; its entry in the stream is its 4-byte mark.  XDRG_CONN_BAD_SIZE
 * (the pre-swap size test of srpc.cc:38-39, or a size that is not a multiple
 * of 4 once the body is there) has no counterpart in msg_sock itself: the
 * next mark would not be word aligned, and every consumer's xdr_get throws
 * xdr_bad_message_size (xdrpp/marshal.h:152-162).
 *
 * Output.  The delivered messages form one contiguous stream in d_out,
 * connections in table order and each connection's messages in wire order:
 * d_offsets[k] is message k's mark, d_offsets[n], d_status->total_bytes and
 * *d_count carry the totals, d_conn_of[k] is message k's connection and, with
 * XDRG_RECV_RPC_SOCK, d_kind[k] is 0 for CALL and 1 for REPLY (d_kind may be
 * NULL without the flag).  d_out and d_offsets are what xdrg_rpc_dispatch,
 * xdrg_rpc_check_replies, xdrg_rpc_match_replies and xdrg_decode_msgs take.
 *
 * Call-level errors, through d_status; neither can occur with out_capacity >=
 * the sum of len and max_msgs >= that sum / 4.  More than max_msgs messages:
 * XDRG_ERR_MSG_COUNT at record max_msgs; *d_count = max_msgs, the first
 * max_msgs entries and d_offsets[max_msgs] are written.  A message that does
 * not fit out_capacity: XDRG_ERR_OVERFLOW_PUT at that message; nothing of it
 * nor of the ones after it is copied.  d_conns is complete in either case (it
 * depends on the walk only), and total_bytes is what the stream needs.
 *
 * XDRG_EINVAL: unknown flags; NULL d_offsets, d_count or d_status; NULL d_segs
 * or d_conns with nconns > 0, d_buf with buf_len > 0, d_out with out_capacity
 * > 0, d_conn_of (with the flag: d_kind) with max_msgs > 0; d_out overlapping
 * d_buf.  XDRG_EALIGN: d_buf, d_out or d_conn_of not 4-aligned, any other
 * array not 8-aligned.  XDRG_EUNSUPPORTED: nconns > 0x7fffffff or max_msgs >=
 * 2^40.  XDRG_ESPACE: workspace below
 * xdrg_rpc_recv_batch_workspace_size(nconns, buf_len), which need not be
 * initialised.  Nothing is allocated, no lock is held; kernels only.
 */
typedef struct xdrg_rpc_conn_in { uint64_t begin; uint64_t len; } xdrg_rpc_conn_in; /* 16 bytes */

enum xdrg_conn_state {
  XDRG_CONN_OPEN = 0,     /* nothing wrong; the tail (if any) waits for more bytes  */
  XDRG_CONN_FRAGMENT = 1, /* fragment bit clear: ECONNRESET      msgsock.cc:86-91   */
  XDRG_CONN_TOO_LONG = 2, /* size > max_msg_len: E2BIG           msgsock.cc:99-117  */
  XDRG_CONN_BAD_SIZE = 3, /* a size no consumer can take (see above)                */
  XDRG_CONN_BAD_RPC = 4   /* XDRG_RECV_RPC_SOCK only: recv_msg's test, msgsock.cc:205-224 */
};

typedef struct xdrg_rpc_conn { /* 32 bytes, one per connection, written for every connection */
  uint64_t first;    /* index of its first message in the batch (exclusive scan of msgs) */
  uint64_t consumed; /* bytes of its segment taken by the delivered messages; on a failure:
                        the failing mark's offset in the segment */
  uint64_t msgs;     /* whole messages delivered */
  uint32_t need;     /* OPEN: 0 if the segment ends at a mark boundary, 4 if it ends inside a
                        mark, 4 + size if it ends inside that message's body; else 0 */
  uint32_t state;    /* enum xdrg_conn_state */
} xdrg_rpc_conn;

#define XDRG_RECV_RPC_SOCK 1u /* flags: apply rpc_sock::recv_msg's test, write d_kind */

size_t xdrg_rpc_recv_batch_workspace_size(uint64_t nconns, uint64_t buf_len);
int xdrg_rpc_recv_batch(const void *d_buf, uint64_t buf_len,
                        const xdrg_rpc_conn_in *d_segs, uint64_t nconns,
                        uint32_t max_msg_len, uint32_t flags,
                        void *d_out, uint64_t out_capacity,
                        uint64_t *d_offsets /* max_msgs + 1 */, uint64_t max_msgs, uint64_t *d_count,
                        uint32_t *d_conn_of /* max_msgs */, uint8_t *d_kind /* max_msgs, or NULL */,
                        xdrg_rpc_conn *d_conns /* nconns */,
                        void *d_workspace, size_t workspace_bytes,
                        xdrg_status *d_status, void *stream);

/* ---------------------------------------------------------------------- */
/* The send side                                                           */
/* ---------------------------------------------------------------------- */
/*
 * msg_sock::putmsg (xdrpp/msgsock.cc:121-134) for the messages of many
 * streams and many connections in one call: the step before writev.  The
 * messages come as up to XDRG_RPC_MAX_SEND_SRCS sources, each a stream of
 * record-marked messages (xdrg_rpc_reply_batch's, xdrg_rpc_call_batch's,
 * xdrg_rpc_recv_batch's d_out) with its offsets and the connection of every
 * entry, in any order: the replies of an asynchronous service in completion
 * order (arpc.h:102-200), calls in application order, a reply stream and a
 * call stream for the same connections (rpc_sock, msgsock.cc:202-232).  They
 * leave as one stream in which every connection's messages are contiguous and
 * in putmsg order, with one queue record per connection: what wqueue_ and
 * wsize_ of a fresh queue would hold, ready for one writev per connection.
 *
 * Order.  Entry k of source s has the global number g = (count_cap of the
 * sources before s) + k; entries at or past min(*d_count, count_cap) of their
 * source are not used.  putmsg order on a connection is ascending g: source 0
 * first, each source in entry order.  The queued messages are sorted by
 * (connection, g), a stable sort whose result depends on the inputs only (no
 * atomic decides a position), and written back to back in d_out.
 *
 * Outcomes.  Every used entry has exactly one, reported in d_pos[g] when d_pos
 * is given (an unused entry reads -2 there and is not counted):
 *   empty     d_offsets[k] == d_offsets[k + 1] (xdrg_rpc_reply_batch's "no
 *             reply", xdrg_rpc_call_batch's "no message"): skipped, -2
 *   unusable  -3: a span with end < begin or end > bytes_len, an offset or a
 *             length that is not a multiple of 4, a length below 4 or above 4
 *             + XDRG_MAX_MSG, a first word that is not BE((length - 4) |
 *             XDRG_MARK_LAST), a connection at or past nconns.  Nothing of
 *             d_bytes past the first word is read for it: what is written to a
 *             socket is always well framed.
 *   dropped   d_closed[conn] != 0, putmsg on a socket with wfail_
 *             (msgsock.cc:124-127): -1
 *   queued    d_pos[g] = its queue position j
 *
 * Outputs.  d_offsets[j] is the mark of queue position j; d_offsets[m],
 * d_status->total_bytes and *d_count carry the totals (m messages).
 * d_conn_of[j] is the connection of position j, d_from[j] = s << 32 | k where
 * it came from.  d_queues[c] is written for every connection, also one with
 * nothing queued (msgs 0, len 0, begin = the end of the connection before
 * it): the ranges of consecutive connections tile the stream.  It depends on
 * the sizes only, not on the copy.  d_counts = {queued, dropped, empty,
 * unusable}, written by a kernel from tile sums.  Entries of d_offsets past m
 * and of d_conn_of / d_from at or past m are unspecified.
 *
 * A capacity below the total is XDRG_ERR_OVERFLOW_PUT at the first queue
 * position that does not fit (record = j, op 0xffff): every message before it
 * is written as in an unbounded call, nothing at or past out_capacity is
 * written, d_queues and d_offsets are complete and total_bytes is what the
 * stream needs.
 *
 * Validated on the host before any HIP call.  XDRG_EINVAL: NULL d_offsets,
 * d_count, d_status; NULL srcs with nsrcs > 0, d_out with out_capacity > 0,
 * d_conn_of or d_from with entries > 0, d_queues with nconns > 0; nsrcs above
 * the limit; a source with count_cap > 0 and NULL d_offsets, or with
 * bytes_len > 0 and NULL d_bytes; d_out overlapping a source's bytes.
 * XDRG_EALIGN: a u64 array, d_queues, d_status or the workspace not 8-aligned;
 * d_out, d_bytes, d_conn, d_conn_of or d_closed not 4-aligned.
 * XDRG_EUNSUPPORTED: entries (the sum of count_cap) above 0xffffffff or nconns
 * above 0x7fffffff.  XDRG_ESPACE: workspace below
 * xdrg_rpc_send_batch_workspace_size(entries, nconns), which need not be
 * initialised.  Zero entries: d_offsets[0], the totals and every queue record
 * are still written.
 *
 * Kernels only: no memset or memcpy node, no wait on the stream, no
 * allocation, no state; capturable on one stream, and the launch sequence does
 * not depend on what the device arrays hold (a batch that is already in
 * connection order skips the sort on the device, not on the host).  Whatever
 * the device arrays hold, nothing outside the given inputs is read and nothing
 * outside the outputs written.  The sort works on XDRG_RPC_SEND_SORT_TILE
 * entries a workgroup.
 */
typedef struct xdrg_rpc_send_src { /* 48 bytes */
  const uint8_t  *d_bytes;   /* a stream of record-marked messages */
  const uint64_t *d_offsets; /* count + 1: entry k = [d_offsets[k], d_offsets[k+1]) */
  const uint32_t *d_conn;    /* count: the connection of entry k; NULL: every entry goes to `conn` */
  const uint64_t *d_count;   /* device count; NULL: count_cap is the count */
  uint64_t bytes_len;
  uint32_t count_cap;        /* host bound, sizes the launch; min(*d_count, count_cap) entries are used */
  uint32_t conn;
} xdrg_rpc_send_src;
#define XDRG_RPC_MAX_SEND_SRCS 64u
#define XDRG_RPC_SEND_SORT_TILE 2048u

typedef struct xdrg_rpc_wqueue { /* 32 bytes, one per connection, written for every connection */
  uint64_t first;  /* queue position of its first message */
  uint64_t msgs;   /* messages queued for it by this call */
  uint64_t begin;  /* its bytes are d_out[begin, begin + len): wsize_ of a fresh queue */
  uint64_t len;
} xdrg_rpc_wqueue;

size_t xdrg_rpc_send_batch_workspace_size(uint64_t entries /* sum of count_cap */, uint64_t nconns);
int xdrg_rpc_send_batch(const xdrg_rpc_send_src *srcs /* HOST */, uint32_t nsrcs,
                        uint64_t nconns, const uint32_t *d_closed /* nconns, or NULL: all open */,
                        void *d_out, uint64_t out_capacity,
                        uint64_t *d_offsets /* entries + 1 */, uint64_t *d_count,
                        uint32_t *d_conn_of /* entries */, uint64_t *d_from /* entries: src << 32 | k */,
                        int64_t *d_pos /* entries, source-major; may be NULL */,
                        xdrg_rpc_wqueue *d_queues /* nconns */, uint64_t *d_counts /* 4, may be NULL */,
                        void *d_workspace, size_t workspace_bytes, xdrg_status *d_status, void *stream);

/* ---------------------------------------------------------------------- */
/* The asynchronous client over many connections                           */
/* ---------------------------------------------------------------------- */
/*
 * In the reference every connection is its own rpc_sock: its own xid_
 * (xdrpp/msgsock.h:118-122; two fresh connections both hand out xid 1), its
 * own calls_ (xdrpp/msgsock.cc:202-232; a reply is looked up in the calls_ of
 * the socket it arrived on, anything else is "ignoring reply to unknown
 * call") and its own abort_all_calls (msgsock.cc:190-200; the calls of the
 * one socket that failed receive NETWORK_ERROR, arpc.h:60-61).  The calls
 * below are xdrg_rpc_next_xids, xdrg_rpc_pending_add, xdrg_rpc_match_replies,
 * xdrg_rpc_call_stats and xdrg_rpc_pending_retire for many rpc_socks at once.
 *
 * The table is two parallel device arrays of ncalls entries: d_calls
 * (xdrg_rpc_call, as above) and d_sock (uint32_t, the entry's socket number),
 * sorted ascending by (sock, xid as unsigned) with no duplicate pair -- the
 * concatenation, in socket order, of the tables the single-socket calls take.
 * Socket numbers are the caller's, 0..nsocks-1, stable across rounds (the rows
 * of xdrg_rpc_recv_batch are per round).  d_call and d_reply_of name positions
 * in this table, and xdrg_rpc_verify_results and xdrg_rpc_gather_results,
 * which read d_calls[c].res only, take it as it is.
 *
 * Every call equals its single-socket sibling applied to each socket's run
 * of the arrays on its own.  All validate on the host before any HIP call
 * (XDRG_EINVAL: NULL required pointers; XDRG_EALIGN: u64 and call arrays not
 * 8-aligned, u32 arrays not 4-aligned; XDRG_ESPACE: a small workspace),
 * launch kernels only (no memset or memcpy node, no wait, no state; capturable
 * on one stream) and neither read nor write outside the given arrays,
 * whatever these hold: a socket number at or past nsocks indexes nothing.
 */

/*
 * get_xid() followed by send_call (msgsock.h:118-122) for a batch of n calls
 * grouped by socket: d_call_sock[k] is call k's socket, non-decreasing.  With
 * [a, b) the run of socket g in d_call_sock and [lo, hi) its run in d_sock,
 * d_xids[k] for a <= k < b is what xdrg_rpc_next_xids(d_calls + lo, hi - lo,
 * d_last[g], b - a, ...) writes at k - a, the skip of a pending 0 included.
 * d_last holds every rpc_sock's xid_.  d_last_out (may be NULL; must not
 * alias d_last) receives xid_ after the batch for EVERY g < nsocks, written by
 * lanes of the call: the last xid of g's run, or d_last[g] when it has none.
 * A call whose socket is >= nsocks counts from 0 over that socket's run of
 * the table.  The call stream itself is xdrg_rpc_call_batch over d_xids,
 * unchanged: with the positions in socket order, socket g's bytes are
 * [d_offsets[a], d_offsets[b]), one writev per connection.
 * XDRG_EINVAL also: ncalls + n > 0xffffffff, nsocks > 0xffffffff, d_last_out
 * equal to or overlapping d_last.  An unsorted d_call_sock gives unspecified
 * xids, in bounds.  n == 0: d_last_out is still written.
 */
int xdrg_rpc_socks_next_xids(const xdrg_rpc_call *d_calls, const uint32_t *d_sock, uint64_t ncalls,
                             const uint32_t *d_last /* nsocks */, uint64_t nsocks,
                             const uint32_t *d_call_sock /* n */, uint64_t n,
                             uint32_t *d_xids /* n */, uint32_t *d_last_out /* nsocks, may be NULL */,
                             void *stream);

/*
 * send_call's emplace (msgsock.cc:227-232) for every socket.  d_new is
 * xdrg_rpc_call_batch's d_sent, d_new_sock the batch's d_call_sock
 * (non-decreasing); within a socket's run the xids ascend with at most one
 * descent (the wrap) and are disjoint from that socket's entries.  Socket g's
 * part of the result is d_merged[lo + a, hi + b): it equals
 * xdrg_rpc_pending_add on that socket's parts, d_merged_sock is g there, and
 * d_old_pos / d_new_pos (may be NULL) are that call's positions plus lo + a.
 * EVERY entry of d_new is merged, XDRG_RPC_RES_UNSENT ones included.  Arrays
 * that break the precondition give an unspecified table inside d_merged and
 * d_merged_sock; a position that would leave them is not written and reads
 * XDRG_RPC_NO_CALL in d_old_pos / d_new_pos.
 * XDRG_EINVAL also: d_merged equal to or overlapping d_calls or d_new,
 * d_merged_sock equal to or overlapping d_sock or d_new_sock.
 * XDRG_EUNSUPPORTED: more than 0x7fffffff workgroups.
 */
int xdrg_rpc_socks_pending_add(const xdrg_rpc_call *d_calls, const uint32_t *d_sock, uint64_t ncalls,
                               const xdrg_rpc_call *d_new /* n */, const uint32_t *d_new_sock /* n */, uint64_t n,
                               xdrg_rpc_call *d_merged /* ncalls + n */, uint32_t *d_merged_sock /* ncalls + n */,
                               uint64_t *d_old_pos /* ncalls, may be NULL */,
                               uint64_t *d_new_pos /* n, may be NULL */, void *stream);

/*
 * rpc_sock::recv_msg (msgsock.cc:202-232) on the socket each message arrived
 * on.  Every rule of xdrg_rpc_match_replies holds (size < 8, CALL, any other
 * word 1, the first reply wins by a 64-bit atomicMin, later replies are
 * XDRG_RPCR_UNKNOWN_XID); the one difference is the lookup key, (sock, word
 * 0), with sock = d_row_sock ? d_row_sock[d_msg_row[i]] : d_msg_row[i].
 * d_msg_row is xdrg_rpc_recv_batch's d_conn_of; d_row_sock (may be NULL) maps
 * the round's rows to socket numbers.  A REPLY whose row is >= nrows, or whose
 * pair is not in the table -- an xid that is pending on another socket
 * included -- is XDRG_RPCR_UNKNOWN_XID with XDRG_RPC_NO_CALL
 * (msgsock.cc:212-216).
 */
int xdrg_rpc_socks_match_replies(const void *d_stream, uint64_t len, const uint64_t *d_offsets, uint64_t n,
                                 const uint32_t *d_msg_row /* n */,
                                 const uint32_t *d_row_sock /* nrows, may be NULL */, uint64_t nrows,
                                 const xdrg_rpc_call *d_calls, const uint32_t *d_sock, uint64_t ncalls,
                                 xdrg_rpc_hdr *d_hdrs, uint64_t *d_call /* n */,
                                 uint64_t *d_reply_of /* ncalls */, void *stream);

/*
 * xdrg_rpc_call_stats with `unanswered` chosen per entry: d_closed[g] nonzero
 * says abort_all_calls (msgsock.cc:190-200) ran on socket g, and a call of g
 * without a reply is {XDRG_RPCS_NETWORK_ERROR, 0} (arpc.h:60-61); on an open
 * socket it is {XDRG_RPCS_PENDING, 0}.  An entry whose socket is >= nsocks
 * counts as open.  A call answered before its socket failed keeps the stat of
 * its reply: recv_msg had erased it (msgsock.cc:217-219) before the failure.
 */
int xdrg_rpc_socks_call_stats(const xdrg_rpc_hdr *d_hdrs, uint64_t n,
                              const uint64_t *d_reply_of /* ncalls */, const uint32_t *d_sock, uint64_t ncalls,
                              const uint32_t *d_closed /* nsocks */, uint64_t nsocks,
                              xdrg_rpc_call_stat *d_stats /* ncalls */, void *stream);

/*
 * Every calls_ after a reply batch: entry j is kept iff d_reply_of[j] ==
 * XDRG_RPC_NO_CALL and its socket is open (d_closed as above).  d_kept and
 * d_kept_sock receive the kept entries in table order, *d_count their number,
 * d_kept_pos[j] (may be NULL) the new position of entry j or
 * XDRG_RPC_NO_CALL.  The three passes of xdrg_rpc_pending_retire (tile
 * counts, one-workgroup scan that writes *d_count, ballot ranks), no atomic,
 * and the same workspace formula.  XDRG_EINVAL also: d_kept equal to or
 * overlapping d_calls, d_kept_sock equal to or overlapping d_sock.
 * XDRG_EUNSUPPORTED: more than 0x7fffffff workgroups.  ncalls == 0: *d_count
 * = 0 is still written, by a kernel.
 */
size_t xdrg_rpc_socks_pending_retire_workspace_size(uint64_t ncalls);
int xdrg_rpc_socks_pending_retire(const xdrg_rpc_call *d_calls, const uint32_t *d_sock, uint64_t ncalls,
                                  const uint64_t *d_reply_of /* ncalls */,
                                  const uint32_t *d_closed /* nsocks */, uint64_t nsocks,
                                  xdrg_rpc_call *d_kept /* ncalls */, uint32_t *d_kept_sock /* ncalls */,
                                  uint64_t *d_kept_pos /* ncalls, may be NULL */, uint64_t *d_count,
                                  void *d_workspace, size_t workspace_bytes, void *stream);

/* Recursion depth per record: d_depths[i] = the deepest class/container
 * level record i's walk enters (the record itself is level 1), so
 * xdr::check_xdr_depth(r_i, limit) (xdrpp/depth_checker.h:72-79) is
 * d_depths[i] <= limit.  A bad union discriminant stops the walk and is
 * reported through d_status like the size pass.  d_heap: the staged heap
 * (element arrays of containers of variable-size elements are read from
 * it; NULL/0 when the plan has none). */
int xdrg_record_depths(const xdrg_plan *plan, const void *d_native, uint64_t n,
                       const void *d_heap, uint64_t heap_len, uint32_t *d_depths,
                       void *d_workspace, size_t workspace_bytes,
                       xdrg_status *d_status, void *stream);

/* Size pass alone: d_sizes[i] = xdr_size(record i) (uint32); d_heap as
 * for xdrg_record_depths.  Both take xdrg_deep_workspace_size(plan, n)
 * bytes of workspace (NULL/0 for every plan that needs none). */
int xdrg_serial_sizes(const xdrg_plan *plan, const void *d_native, uint64_t n,
                      const void *d_heap, uint64_t heap_len, uint32_t *d_sizes,
                      uint32_t stack_limit, void *d_workspace, size_t workspace_bytes,
                      xdrg_status *d_status, void *stream);

/* ---------------------------------------------------------------------- */
/* Comparison: operator== and operator<=> of record batches                */
/* ---------------------------------------------------------------------- */
/*
 * xdrg_compare <- xdr::operator== / operator<=> of xdrpp/types.h:946-1062
 * (XDRPP_STRONG_ORDER = 0) and pointer's at :647-657, for n record pairs:
 * structs field by field in declaration order, the first field that is not
 * equivalent deciding (types.h:1047-1056); unions by discriminant, then by
 * the active arm (:1030-1044; equal discriminants that select a void arm or
 * no arm compare equivalent); an absent pointer less than a present one
 * (:651-657); xvector / xarray as std::vector / std::array (lexicographic,
 * then the shorter is less); opaque and string bytes as unsigned chars, then
 * by length; integers by value with their signedness, enums as int32, bools
 * false < true (any nonzero native byte is true), float and double as IEEE
 * values (-0.0 equivalent to +0.0, a NaN unordered against everything).
 * Native padding never influences a result.
 *
 * The plan ops do not say whether a word is signed, unsigned or IEEE, so a
 * plan carries its value classes in a side table beside the ops (the ops
 * themselves, and everything computed from them, stay as they are):
 * xdrg_plan_set_compare_classes takes one byte per op -- meaningful on U32,
 * U64 and UNION ops (the discriminant's class; XDRG_CLASS_BOOL marks a bool
 * discriminant); an ENUM op is always signed.  XDRG_EINVAL for a wrong nops
 * or a value out of range.  Host-only; set before the plan's first
 * xdrg_compare and before the plan is shared between threads.
 */
enum xdrg_compare_class {
  XDRG_CLASS_UNSIGNED = 0,
  XDRG_CLASS_SIGNED = 1,
  XDRG_CLASS_IEEE = 2,
  XDRG_CLASS_BOOL = 3 /* UNION ops only */
};
int xdrg_plan_set_compare_classes(xdrg_plan *plan, const uint8_t *classes, uint32_t nops);

enum xdrg_cmp {
  XDRG_CMP_LESS = -1,
  XDRG_CMP_EQUAL = 0,     /* a == b holds exactly when the result is this */
  XDRG_CMP_GREATER = 1,
  XDRG_CMP_UNORDERED = 2, /* std::partial_ordering::unordered */
  XDRG_CMP_DEEP = 3,      /* the pair is equal down to a container that would need more than
                             XDRG_SUB_FRAMES open element frames: not compared */
  XDRG_CMP_BADREF = 4     /* a bytes or element reference of a or b (with a nonzero length or
                             count) points outside its heap; nothing is read through it */
};
/*
 * d_result[i] = a[i] <=> b[i] (int8, enum xdrg_cmp).  d_a and d_b are native
 * record batches of the plan's stride, each with its own heap (the staging
 * heap, or the heap a decode returned; NULL/0 for plans without references).
 * Host checks first, then kernels only (no memset, no sync, no allocation
 * after the plan's first compare on the device, which uploads its tables):
 * capturable.  n = 0 launches nothing.  XDRG_EINVAL: null arguments;
 * XDRG_EALIGN: a native base or heap xdrg_encode would refuse (fixed plans:
 * 4-byte aligned records; var plans: 8-byte aligned records, 4-byte aligned
 * heaps); XDRG_EUNSUPPORTED: the plan has U32, U64 or UNION ops and no
 * classes.  Fixed plans whose native stride is a multiple of 16 (and whose
 * batches are 16-byte aligned) are compared chunk by chunk, a lane per
 * 16-byte chunk position; everything else by one lane walking the pair.
 */
int xdrg_compare(const xdrg_plan *plan, const void *d_a, const void *d_a_heap, uint64_t a_heap_len,
                 const void *d_b, const void *d_b_heap, uint64_t b_heap_len, uint64_t n,
                 int8_t *d_result, void *stream);

/*
 * xdrg_sort <- std::stable_sort and std::unique of a batch by xdr::operator<
 * (xdrpp/types.h:946-1062, XDRPP_STRONG_ORDER = 0), as a permutation: no
 * record moves.  d_recs is one native batch of the plan's stride with its
 * heap, as one side of xdrg_compare.
 *
 * Record i is sortable when rec[i] <=> rec[i] is XDRG_CMP_EQUAL under
 * xdrg_compare's rules: not a record that holds a NaN in a field its own walk
 * reaches, nor one with a reference outside the heap (BADREF), nor one nested
 * past the register frames (DEEP); xdrg_compare(recs, recs) tells which.
 * With m the number of sortable records:
 *
 *   d_perm[0..m)   the sortable records' indices in the order std::stable_sort
 *                  gives them: ascending, equivalent records in input order --
 *                  the one ascending order of the keys (record, index)
 *   d_perm[m..n)   the other records' indices, in input order
 *   d_first[k]     (may be NULL) k < m: 1 if k == 0 or rec[perm[k-1]] <
 *                  rec[perm[k]], else 0 -- a 1 starts a group of equivalent
 *                  records (std::unique, the contents of a std::set);
 *                  k >= m: 1 (such a record equals nothing, itself included)
 *   d_counts[0]    m
 *   d_counts[1]    the ones in d_first[0..m): the distinct values (computed
 *                  with or without d_first)
 *
 * Host checks first, before any HIP call: XDRG_EINVAL for a null plan, or
 * with n > 0 null records, perm, counts or workspace, for a heap length
 * without a heap, for workspace_bytes below xdrg_sort_workspace_size(plan,
 * n); XDRG_EALIGN for records or a heap xdrg_compare would refuse, a
 * workspace that is not 16-byte aligned, a d_perm that is not 4-byte or
 * d_counts that is not 8-byte aligned; XDRG_EUNSUPPORTED for n > 2^31 (the
 * size is 0 then) and for a plan with U32, U64 or UNION ops and no classes.
 * n = 0 launches nothing and writes nothing.
 *
 * Then kernels only (no memset, no memcpy, no sync, no allocation after the
 * plan's first compare or sort on the device, which uploads the class
 * table): capturable.  The number of launches depends on n alone; m is never
 * read on the host.  Every store is in bounds whatever the bytes of the
 * batch.  Every plan sorts by the pair walk, ceil(log2 n) merge passes by
 * rank, the first eight in one launch.
 */
size_t xdrg_sort_workspace_size(const xdrg_plan *plan, uint64_t n);
int xdrg_sort(const xdrg_plan *plan, const void *d_recs, const void *d_heap, uint64_t heap_len, uint64_t n,
              uint32_t *d_perm, uint8_t *d_first /* may be NULL */, uint64_t *d_counts /* [2] */,
              void *d_workspace, size_t workspace_bytes, void *stream);

/* Bulk big-endian swaps (endian.h swap32/swap64) over device arrays. */
int xdrg_swap32(const uint32_t *d_in, uint32_t *d_out, uint64_t n, void *stream);
int xdrg_swap64(const uint64_t *d_in, uint64_t *d_out, uint64_t n, void *stream);

/* what() string and exception class of a data error.  For
 * XDRG_ERR_BAD_DISCRIMINANT the reference message names the union
 * ("bad value of <tag> in <union>"); the C++/Python layers format it from
 * the op's name id, this returns the generic prefix. */
const char *xdrg_error_message(int code);
int xdrg_error_exception(int code);

/* Last HIP error string recorded by this thread (for XDRG_EHIP). */
const char *xdrg_last_hip_error(void);

#ifdef __cplusplus
}
#endif

#endif /* XDRGPU_H_INCLUDED */
