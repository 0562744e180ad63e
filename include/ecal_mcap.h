/*
 * ecal_mcap.h — mcap ingest: ROS 2 MCAP recordings of event messages into packed records, decoded in HBM (libecal.so, the same
 * library as ecal.h; ABI version unchanged; nothing in ecal.h calls these, and the bag ingest keeps refusing an MCAP file by name).
 *
 * The file that `ros2 bag record` writes by default, of a camera driven by libcaer_driver / dvs_msgs (iniVation) or by
 * metavision_driver / event_camera_msgs (Prophesee), without a host converter in front.  Nothing in the reference reads MCAP, and no
 * MCAP library, no ROS 2 and no real recording was at hand when this was written: the container is restated from the published MCAP
 * specification, the message layout from the published CDR rules (XCDR version 1, as rmw writes it) and from the message
 * definition the file itself carries, and the MONO bit layout in particular is restated from memory of event_camera_codecs.  This
 * contract is the specification (eventcalib_amd/csrc/mcap_events.hpp restates it for the kernels, the host decoder and the tests).
 * The first real file has to be checked against `ros2 topic echo`: the event count, the first and last stamps, a handful of
 * coordinates.  Compressed chunks, SQLite .db3 bags, libcaer_cmp and evt2 packets, big-endian CDR and stereo files without a chosen
 * topic are refused by name.
 *
 * File: the 8 bytes "\x89MCAP0\r\n", then a chain of records: u8 opcode, u64 length, `length` bytes of content.  All integers are
 *   little-endian; a string is a u32 length and that many bytes.  Anything else in front is ECAL_ERR_INVALID (a ROS 1 bag and an
 *   SQLite file by name).  Error texts name the record's number (0-based, over all records, inner and outer, in file order) and its
 *   byte offset in the file.  By opcode:
 *     0x01 header, 0x02 footer: stepped over.
 *     0x03 schema:  u16 id, string name, string encoding, u32 len + data (the message definition).
 *     0x04 channel: u16 id, u16 schema_id, string topic, string message_encoding, u32 len + metadata.  schema_id 0 is "no schema";
 *          any other must be defined in front of the channel.
 *     0x05 message: u16 channel_id, u32 sequence, u64 log_time, u64 publish_time; the rest of the record is the data.  A message
 *          whose channel is not defined in front of it is ECAL_ERR_INVALID.  At top level (an unchunked file) and inside chunks.
 *     0x06 chunk:   u64 start, u64 end, u64 uncompressed_size, u32 crc, string compression, u64 len + records.  len must be the rest
 *          of the record.  Compression "": the records are a chain walked in turn, of which only 0x03, 0x04 and 0x05 are allowed
 *          (any other opcode there is ECAL_ERR_INVALID, and so is an inner record that runs past the end of a chunk that is
 *          wholly present).  Any other compression ("lz4", "zstd") is ECAL_ERR_INVALID with a text that names it and says to
 *          rewrite the file uncompressed (`ros2 bag convert` or the mcap command line tool can; or record without compression).
 *     0x07 .. 0x0E (message index, chunk index, attachment, attachment index, statistics, metadata, metadata index, summary offset):
 *          stepped over.  The summary section is never relied on.
 *     0x0F data end: the chain ends here; nothing behind it is interpreted (a footer ends the chain too).
 *     Any other opcode in front of data end is ECAL_ERR_INVALID.
 *   A schema or a channel that is seen again must repeat its content byte for byte (else ECAL_ERR_INVALID).  CRCs are stepped over.
 *   A record whose 9 header bytes or whose content runs past the end of the file ends the chain, like a recording cut short: of a
 *   chunk cut short the inner records wholly present are walked; a message cut short is not decoded at all (nor counted).
 *   n_trailing_bytes = the bytes from the start of the first record (inner or outer) that is not wholly present.  A file that never
 *   got a data end or a footer reads the same as a closed one.
 * Which messages carry events: a channel is chosen when its message_encoding is "cdr", its schema's encoding is "ros2msg" and the
 *   schema's text declares a top-level field `events`.  A channel of encoding "cdr" whose schema is "ros2idl" and speaks of `events`
 *   is ECAL_ERR_INVALID with a text that names ros2idl.  With options.topic non-empty only channels of that topic are looked at;
 *   with it empty all chosen channels must share one topic: two or more event topics without a choice (a stereo file) is
 *   ECAL_ERR_INVALID with a text that lists them.  No chosen channel at all is ECAL_ERR_INVALID with a text that lists the topics
 *   and schema names that are there.  Every message of another channel is counted in n_other_messages.
 * Layout, from the file's own schema text (ros2msg), not from remembered field orders: lines `type name [default]`; `#` opens a
 *   comment; a line with `=` behind the type is a constant and is skipped; a line of `=` signs (three or more) ends a definition
 *   and the line `MSG: pkg/Type` behind it opens a dependency's.  The top-level fields are taken in order.  Types: bool byte char
 *   int8 uint8 (1 byte), int16 uint16 (2), int32 uint32 float32 (4), int64 uint64 float64 (8), string (also string<=N), T[N], T[]
 *   and T[<=N] of these primitives; std_msgs/Header (a Time, then the string frame_id) and builtin_interfaces/Time (int32 sec,
 *   uint32 nanosec) are built in, under any package prefix.  Any other type at top level beside `events` is ECAL_ERR_INVALID by name.
 *   CDR: the data starts with a 4-byte encapsulation header; 00 01 xx xx is little-endian CDR; 00 00 (big-endian CDR), 00 02 / 00 03
 *   (PL_CDR) and 00 06 .. 00 0B (XCDR2) are refused by name, any other value too.  Every primitive is aligned to its own size,
 *   counted from byte 4 of the data.  A string is a u32 length that includes the NUL, then the bytes.  A sequence is a u32 count,
 *   then the elements (no padding in front of the elements of an empty sequence).  The walk over all top-level fields must end
 *   within the data and within 3 bytes of its length; else the message is ECAL_ERR_INVALID (this catches a foreign layout).
 * Three kinds; a file has one, mixed kinds (and two STRUCT layouts) are refused:
 *   ECAL_MCAP_STRUCT  `events` is a sequence of a message type whose definition stands among the dependencies (matched by its last
 *     name component) and has exactly: x and y (uint8 / uint16 / uint32, or byte / char), polarity or p (any 1-byte type), and ts, t
 *     or stamp of type Time, in any order.  Any other field is ECAL_ERR_INVALID with the types listed.  This is
 *     dvs_msgs/msg/EventArray and prophesee_event_msgs.  CDR pads no struct tail, so event 0 (which starts 4-byte aligned, behind
 *     the count) and the later events differ: for dvs_msgs/Event (uint16 x, uint16 y, Time ts, bool polarity) event 0 has
 *     x 0, y 2, sec 4, nanosec 8, polarity 12; event k >= 1 starts lead + stride (k - 1) = 14 + 16 (k - 1) bytes on and has x 0, y 2,
 *     sec 6, nanosec 10, polarity 14.  The indexer derives both offset sets, lead and stride from the schema by laying out eight
 *     events, checks that stride and offsets are constant from event 1 on, and reports them in info.layout.
 *     t_ns = (int64) sec * 1 000 000 000 + nanosec with sec SIGNED; polarity = byte != 0.  msg_width / msg_height: the first chosen
 *     message's top-level integer fields `width` / `height` when it has them, else 0.
 *   ECAL_MCAP_MONO    `events` is uint8[] (an event_camera_msgs/msg/EventPacket-shaped message); the integer fields time_base,
 *     width and height, the string encoding and the 1-byte is_bigendian are found by name and must all be there.
 *     encoding == "mono": one little-endian 64-bit word an event, dt = bits 31..0 (nanoseconds), x = bits 47..32, y = bits 62..48,
 *     polarity = bit 63; t_ns = time_base + dt (time_base's 64 bits taken as int64).  is_bigendian != 0 and a byte count that is
 *     not a multiple of 8 are ECAL_ERR_INVALID.
 *   ECAL_MCAP_EVT3    the same message with encoding == "evt3": the messages' byte arrays, in file order, are ONE EVT3 payload (the
 *     raw ingest's, ecal.h): the decoder state runs across message boundaries, as it does in the camera.  A message with an odd byte
 *     count is ECAL_ERR_INVALID.  Time is the camera's clock, as in the raw ingest.
 *   Any other encoding string ("libcaer", "libcaer_cmp", "evt2", ...) is ECAL_ERR_INVALID by name.
 * Conversion and filter, STRUCT and MONO — the bag ingest's, word for word: t = (double)(t_ns - time_base) * 1e-9; with width /
 *   height non-zero an event with x >= width or y >= height is dropped (n_outside); flip_x / flip_y give width - 1 - x /
 *   height - 1 - y BEHIND the bounds test and need width / height; then t < 0 is dropped (n_negative); then kept if t >= start_time
 *   (else n_before_start), and with has_end_time the first event with t >= end_time ends the stream: it and every event behind it
 *   count as n_after_end and as nothing else.  n_events + n_outside + n_negative + n_before_start + n_after_end = n_raw_events.
 *   EVT3: the raw ingest's conversion and filter (microseconds), then the flips on the kept records are NOT available: flip_x /
 *   flip_y with EVT3 are ECAL_ERR_INVALID.  There n_raw_events = the five counters + n_no_state (the indexer reports 0: it does not
 *   decode words).
 * Time base: options.auto_time_base (default 1): STRUCT: sec * 1 000 000 000 of the first event, in file order, of the first chosen
 *   message that has events; MONO: floor((time_base + dt) / 1e9) * 1e9 of that event; the indexer reports it as first_stamp_ns (0
 *   when no message has events).  EVT3: 0.  With auto_time_base == 0 options.time_base is taken: int64 nanoseconds of epoch time
 *   (STRUCT, MONO), microseconds of the camera's clock (EVT3).  info.time_base = the base in force.  The _dev entry point takes an
 *   explicit base only: auto_time_base != 0 there is ECAL_ERR_INVALID.
 *
 * Table entry (ecal_mcap_message, 24 bytes, file order; also one for a message of no events): offset = of the message's event 0
 *   (STRUCT, MONO) or of its first payload byte (EVT3), from byte 0 of the file; n = events (STRUCT, MONO) or payload bytes (EVT3);
 *   reserved = 0; time_base_ns = the message's time_base (MONO only, else 0).  NO alignment of anything in the file may be assumed.
 *
 * ecal_mcap_block_events: event slots per decode block of this build — a fact for tests that place block boundaries.
 * ecal_mcap_index_messages: a HOST function over the file's bytes in host memory; ctx may be NULL (no error text then); opt (may be
 *   NULL): only topic is looked at.  *n_messages = the count; ECAL_ERR_RANGE when it exceeds `capacity` (out holds the first
 *   `capacity`; out may be NULL with capacity 0: a count).  info (optional) is filled on ECAL_OK and ECAL_ERR_RANGE: n_messages,
 *   n_other_messages, n_chunks, n_schemas, n_channels, n_raw_events (STRUCT, MONO), n_payload_bytes (EVT3), n_trailing_bytes,
 *   msg_width, msg_height, first_stamp_ns, kind and layout (for MONO: lead = stride = span = 8; for EVT3 all zero but the kind).
 * ecal_mcap_count_events_dev: *n_events (HOST) = the events before any drop (STRUCT, MONO: the table's sum; EVT3: the events the
 *   gathered payload's words emit): always a sufficient `capacity`.  Waits for `stream`.
 * ecal_events_from_mcap_dev: d_file (DEVICE, 16-byte aligned, the whole file, n_bytes bytes; nothing behind n_bytes is read),
 *   d_messages (DEVICE, 8-byte aligned, entries as the indexer writes them) and layout (HOST, the indexer's) into d_events (DEVICE,
 *   room for `capacity` records, any alignment, file order, not sorted).  opt->topic is not looked at.  A table entry that does not
 *   lie within the file is ECAL_ERR_INVALID, and nothing outside the file is loaded.  info (HOST) is filled on ECAL_OK and on
 *   ECAL_ERR_RANGE (capacity too small: info->n_events = the count needed, call again; also more than 2^32-1 events); what the
 *   indexer reports (n_other_messages, n_chunks, n_schemas, n_channels, n_trailing_bytes, msg_width / msg_height, first_stamp_ns)
 *   is not this call's.  On an error the contents of d_events are undefined.  Enqueues on `stream` and waits for it.
 * ecal_stream_create_from_mcap_file: the file through pinned buffers into HBM, the table built on the host beside the upload,
 *   decoded on the device, the file's bytes freed, then the stream brought into time order if it is not.  info may be NULL.
 * ecal_mcap_to_bin_file: the same records in file order, no sort, as a .bin of the reference's layout.
 */
#ifndef ECAL_MCAP_H_
#define ECAL_MCAP_H_

#include "ecal.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { ECAL_MCAP_NONE = 0, ECAL_MCAP_STRUCT = 1, ECAL_MCAP_MONO = 2, ECAL_MCAP_EVT3 = 3 };

typedef struct ecal_mcap_options {
    const char *topic;       /* NULL or "": every chosen channel (they must share one topic) */
    int auto_time_base;      /* 1: the base is the first event's whole second (EVT3: 0) */
    int64_t time_base;       /* with auto_time_base == 0: nanoseconds of epoch time (EVT3: microseconds of the camera's clock) */
    uint32_t width, height;  /* 0: no bound */
    int flip_x, flip_y;      /* need width / height; STRUCT and MONO only */
    double start_time;       /* seconds */
    int has_end_time;
    double end_time;         /* seconds */
} ecal_mcap_options;

typedef struct ecal_mcap_layout {
    uint32_t kind;           /* ECAL_MCAP_*; ECAL_MCAP_NONE: no chosen message told it yet (a packet channel without messages) */
    uint32_t lead;           /* bytes from event 0 to event 1 */
    uint32_t stride;         /* bytes from event k to event k + 1, k >= 1 */
    uint32_t span[2];        /* bytes from an event's start to the end of its last field: event 0, later events */
    uint8_t x[2], y[2], sec[2], nsec[2], pol[2]; /* STRUCT: byte offsets of the fields in event 0, in later events */
    uint8_t x_bytes, y_bytes;                    /* STRUCT: 1, 2 or 4 */
} ecal_mcap_layout;

typedef struct ecal_mcap_info {
    uint64_t n_raw_events;     /* events before any drop */
    uint64_t n_events;         /* records written, or needed */
    uint64_t n_outside;        /* events dropped for x >= width or y >= height */
    uint64_t n_negative;       /* events dropped for t < 0 */
    uint64_t n_before_start;   /* events dropped for t < start_time */
    uint64_t n_after_end;      /* events from the one that ended the stream on */
    uint64_t n_messages;       /* chosen messages (also those of no events) */
    uint64_t n_other_messages; /* messages of other channels */
    uint64_t n_chunks;
    uint64_t n_schemas;        /* distinct schema ids */
    uint64_t n_channels;       /* distinct channel ids */
    uint64_t n_trailing_bytes; /* bytes from the first record that is not wholly present */
    int64_t first_stamp_ns;    /* the automatic base of STRUCT and MONO */
    int64_t time_base;         /* the base in force */
    uint32_t msg_width, msg_height; /* the first chosen message's own; may differ from the options */
    uint64_t n_payload_bytes;  /* EVT3: bytes of the gathered payload */
    uint64_t n_no_state;       /* EVT3: the raw ingest's */
    uint64_t n_other_words;    /* EVT3: the raw ingest's */
    uint64_t n_time_wraps;     /* EVT3: the raw ingest's */
    ecal_mcap_layout layout;   /* the kind in force is layout.kind */
} ecal_mcap_info;

typedef struct ecal_mcap_message {
    uint64_t offset;       /* of event 0 / of the first payload byte, from byte 0 of the file */
    uint32_t n;            /* events (STRUCT, MONO) or payload bytes (EVT3) */
    uint32_t reserved;     /* 0 */
    int64_t time_base_ns;  /* MONO: the message's time_base; else 0 */
} ecal_mcap_message;

void ecal_mcap_default_options(ecal_mcap_options *opt);
uint32_t ecal_mcap_block_events(void);
int ecal_mcap_index_messages(ecal_ctx *ctx, const uint8_t *file_host, uint64_t n_bytes, const ecal_mcap_options *opt, ecal_mcap_message *out,
                             uint64_t capacity, uint64_t *n_messages, ecal_mcap_info *info);
int ecal_mcap_count_events_dev(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const ecal_mcap_message *d_messages,
                               uint64_t n_messages, const ecal_mcap_layout *layout, uint64_t *n_events, void *stream);
int ecal_events_from_mcap_dev(ecal_ctx *ctx, const uint8_t *d_file, uint64_t n_bytes, const ecal_mcap_message *d_messages,
                              uint64_t n_messages, const ecal_mcap_layout *layout, const ecal_mcap_options *opt,
                              uint8_t *d_events /*room for capacity records*/, uint64_t capacity, ecal_mcap_info *info, void *stream);
int ecal_stream_create_from_mcap_file(ecal_ctx *ctx, const char *path, const ecal_mcap_options *opt, ecal_stream **out, ecal_mcap_info *info);
int ecal_mcap_to_bin_file(ecal_ctx *ctx, const char *mcap_path, const char *bin_path, const ecal_mcap_options *opt, ecal_mcap_info *info);

#ifdef __cplusplus
}
#endif
#endif /* ECAL_MCAP_H_ */
