// Host-side counterparts of the reference's event module (modules/camera_calibration/event) on top
// of libecal.so: same class names and member meaning, Eigen/OpenCV-free.
//   opengv2::Event          event/include/opengv2/event/Event.hpp
//   opengv2::EventStream    event/include/opengv2/event/EventStream.hpp, event/src/EventStream.cpp
//   opengv2::EventContainer event/include/opengv2/event/EventContainer.hpp  (device-resident here)
//   opengv2::EventFrame     event/include/opengv2/event/EventFrame.hpp, event/src/EventFrame.cpp
#ifndef ECAL_HOST_EVENT_HPP_
#define ECAL_HOST_EVENT_HPP_

#include <array>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/ecal.h"
#include "../raw_events.hpp"
#include "../aedat_events.hpp"
#include "../aedat4_events.hpp"
#include "../bag_events.hpp"
#include "../mcap_events.hpp"
#include "../../../include/ecal_mcap.h"
#include "../fields_events.hpp"
#include "dbscan.h"

namespace opengv2 {

using Vector2d = std::array<double, 2>;  // stands in for Eigen::Vector2d: operator[] and contiguous

class Event {
public:
    Event() : timeStamp_(0), location_{{0, 0}}, polarity_(false) {}
    Event(double timeStamp, const Vector2d &location, bool polarity)
        : timeStamp_(timeStamp), location_(location), polarity_(polarity) {}
    double timeStamp() const noexcept { return timeStamp_; }
    const Vector2d &location() const noexcept { return location_; }  // (x, y)
    bool polarity() const noexcept { return polarity_; }             // true = positive

    static constexpr size_t kRecordBytes = 25;  // f64 t, f64 x, f64 y, u8 polarity — packed
    static Event unpack(const uint8_t *r) {
        Event e;
        std::memcpy(&e.timeStamp_, r, 8);
        std::memcpy(&e.location_[0], r + 8, 8);
        std::memcpy(&e.location_[1], r + 16, 8);
        e.polarity_ = r[24] != 0;
        return e;
    }

private:
    double timeStamp_;
    Vector2d location_;
    bool polarity_;
};

// Single-pass reader of the reference's .bin format.  Throws std::invalid_argument when the file
// does not exist, like the reference constructor (EventStream.cpp:10-17).
class EventStream {
public:
    explicit EventStream(const std::string &binFilePath) : is_(binFilePath, std::ifstream::binary | std::ifstream::in) {
        if (!is_.is_open()) throw std::invalid_argument("No such file: " + binFilePath);
        advance();
    }
    void close() {
        if (is_.is_open()) is_.close();
        end_ = true;
    }
    bool isEnd() const noexcept { return end_; }
    const Event &current() const noexcept { return cur_; }
    const uint8_t *currentRecord() const noexcept { return rec_; }
    void next() { advance(); }

    // text -> .bin converter with the reference's rules (EventStream.cpp:25-67): lines
    // "stamp x y polarity"; t = (stamp - base) * magnitude; negative t dropped; stops after endTime.
    static long long txt2bin(const std::string &txtFilePath, double timeMagnitude = 1e-6,
                             long long timeBase_in = std::numeric_limits<long long>::min(),
                             long long endTime_in = std::numeric_limits<long long>::min()) {
        std::ifstream is(txtFilePath);
        if (!is.is_open()) throw std::invalid_argument("No such file: " + txtFilePath);
        const auto dot = txtFilePath.find_last_of('.');
        std::ofstream os(txtFilePath.substr(0, dot) + ".bin", std::ofstream::binary | std::ofstream::trunc);
        long long counter = 0, stamp = 0, base = timeBase_in;
        double x = 0, y = 0;
        bool pol = false;
        while (is.good()) {
            is >> stamp >> x >> y >> pol;
            if (counter == 0 && timeBase_in == std::numeric_limits<long long>::min()) base = stamp;
            if (endTime_in != std::numeric_limits<long long>::min() && stamp > endTime_in) break;
            const double t = (stamp - base) * timeMagnitude;
            if (t < 0) continue;
            os.write((const char *) &t, 8);
            os.write((const char *) &x, 8);
            os.write((const char *) &y, 8);
            os.write((const char *) &pol, 1);
            counter++;
        }
        return counter;
    }
    // txt2bin on the device (ecal_text_to_bin_file: the text uploaded and parsed in HBM): the same arguments, the same output
    // file name, the same bytes in it for a text of one record per line, the same returned count.  A malformed line throws
    // std::invalid_argument naming it (the reference stops silently there and writes a record of stale values).
    static long long txt2binDevice(const std::string &txtFilePath, double timeMagnitude = 1e-6,
                                   long long timeBase_in = std::numeric_limits<long long>::min(),
                                   long long endTime_in = std::numeric_limits<long long>::min()) {
        const ecal_text_options opt = textOptions(timeMagnitude, timeBase_in, endTime_in);
        const auto dot = txtFilePath.find_last_of('.');
        ecal_text_info info;
        ecal_ctx *ctx = ecal_host::thread_ctx();
        const int rc = ecal_text_to_bin_file(ctx, txtFilePath.c_str(), (txtFilePath.substr(0, dot) + ".bin").c_str(), &opt, &info);
        if (rc == ECAL_ERR_INVALID) throw std::invalid_argument(std::string("txt2binDevice: ") + ecal_last_error(ctx));
        if (rc != ECAL_OK) throw std::runtime_error(std::string("ecal_text_to_bin_file: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        return (long long) info.n_events;
    }
    // A Prophesee .raw recording (EVT3 / EVT2; include/ecal.h, "raw ingest") -> .bin beside it, on one host thread: the header,
    // then the plain sequential decoder of raw_events.hpp, the records in file order.  The baseline of raw2binDevice, and its
    // check: both write the same bytes.  opt null: the defaults (format from the header, the camera's clock, no bounds).
    static long long raw2bin(const std::string &rawFilePath, const ecal_raw_options *opt = nullptr, ecal_raw_info *info = nullptr) {
        std::ifstream is(rawFilePath, std::ifstream::binary);
        if (!is.is_open()) throw std::invalid_argument("No such file: " + rawFilePath);
        is.seekg(0, std::ifstream::end);
        std::vector<uint8_t> bytes((size_t) is.tellg());
        is.seekg(0);
        is.read((char *) bytes.data(), (std::streamsize) bytes.size());
        if ((size_t) is.gcount() != bytes.size()) throw std::runtime_error("raw2bin: cannot read " + rawFilePath);
        ecal_raw_options o;
        if (opt) o = *opt; else ecal_raw_default_options(&o);
        int headerFormat = ECAL_RAW_AUTO;
        uint64_t headerBytes = 0;
        (void) ecal_raw::raw_parse_header(bytes.data(), bytes.size(), true, &headerFormat, &headerBytes);
        const int format = o.format != ECAL_RAW_AUTO ? o.format : headerFormat;
        if (format != ECAL_RAW_EVT2 && format != ECAL_RAW_EVT3) throw std::invalid_argument("raw2bin: no format option and no format line in the header of " + rawFilePath);
        const ecal_raw::RawFilter f{o.time_base, o.width, o.height, o.start_time, o.has_end_time, o.end_time};
        ecal_raw::RawCounts c;
        std::vector<uint8_t> out;
        auto put = [&](const uint8_t *rec) { out.insert(out.end(), rec, rec + Event::kRecordBytes); };
        const uint8_t *payload = bytes.data() + headerBytes;
        const uint64_t n = bytes.size() - headerBytes;
        if (format == ECAL_RAW_EVT3) ecal_raw::raw_decode_sequential<ecal_raw::Evt3>(payload, n, f, c, put);
        else ecal_raw::raw_decode_sequential<ecal_raw::Evt2>(payload, n, f, c, put);
        const auto dot = rawFilePath.find_last_of('.');
        std::ofstream os(rawFilePath.substr(0, dot) + ".bin", std::ofstream::binary | std::ofstream::trunc);
        os.write((const char *) out.data(), (std::streamsize) out.size());
        if (info)
            *info = ecal_raw_info{c.n_words, c.n_events, c.n_no_state, c.n_outside, c.n_negative, c.n_before_start, c.n_after_end,
                                  c.n_other_words, c.n_trailing_bytes, c.n_time_wraps, format, headerBytes};
        return (long long) c.n_events;
    }
    // raw2bin on the device (ecal_raw_to_bin_file: the payload uploaded and decoded in HBM): the same arguments, the same output
    // file name, the same bytes in it, the same returned count
    static long long raw2binDevice(const std::string &rawFilePath, const ecal_raw_options *opt = nullptr, ecal_raw_info *info = nullptr) {
        const auto dot = rawFilePath.find_last_of('.');
        ecal_raw_info I;
        ecal_ctx *ctx = ecal_host::thread_ctx();
        const int rc = ecal_raw_to_bin_file(ctx, rawFilePath.c_str(), (rawFilePath.substr(0, dot) + ".bin").c_str(), opt, &I);
        if (rc == ECAL_ERR_INVALID) throw std::invalid_argument(std::string("raw2binDevice: ") + ecal_last_error(ctx));
        if (rc != ECAL_OK) throw std::runtime_error(std::string("ecal_raw_to_bin_file: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        if (info) *info = I;
        return (long long) I.n_events;
    }
    // An iniVation .aedat recording (AEDAT 3.1 / 2.0; include/ecal.h, "aedat ingest") -> .bin beside it, on one host thread: the
    // header, then the plain sequential decoder of aedat_events.hpp, the records in file order.  The baseline of aedat2binDevice,
    // and its check: both write the same bytes.  opt null: the defaults (version from the first line, every source, the camera's
    // clock, no bounds, no flips).
    static long long aedat2bin(const std::string &aedatFilePath, const ecal_aedat_options *opt = nullptr, ecal_aedat_info *info = nullptr) {
        std::ifstream is(aedatFilePath, std::ifstream::binary);
        if (!is.is_open()) throw std::invalid_argument("No such file: " + aedatFilePath);
        is.seekg(0, std::ifstream::end);
        std::vector<uint8_t> bytes((size_t) is.tellg());
        is.seekg(0);
        is.read((char *) bytes.data(), (std::streamsize) bytes.size());
        if ((size_t) is.gcount() != bytes.size()) throw std::runtime_error("aedat2bin: cannot read " + aedatFilePath);
        ecal_aedat_options o;
        if (opt) o = *opt; else ecal_aedat_default_options(&o);
        if ((o.flip_x && !o.width) || (o.flip_y && !o.height)) throw std::invalid_argument("aedat2bin: flip_x / flip_y need width / height");
        int format = ECAL_AEDAT_AUTO;
        uint64_t headerBytes = 0;
        std::string err;
        const size_t headBytes = std::min<size_t>(bytes.size(), (size_t) 1 << 20);   // (the header lies within the first MiB)
        if (ecal_aedat::aedat_parse_header(bytes.data(), headBytes, headBytes == bytes.size(), o.format, &format, &headerBytes, &err))
            throw std::invalid_argument("aedat2bin: " + err + " (" + aedatFilePath + ")");
        const ecal_aedat::AedatFilter f{o.time_base, o.width, o.height, o.start_time, o.has_end_time, o.end_time, o.flip_x, o.flip_y};
        ecal_aedat::AedatCounts c;
        std::vector<uint8_t> out;
        auto put = [&](const uint8_t *rec) { out.insert(out.end(), rec, rec + Event::kRecordBytes); };
        const uint8_t *payload = bytes.data() + headerBytes;
        const uint64_t n = bytes.size() - headerBytes;
        if (format == ECAL_AEDAT_3_1) {
            if (ecal_aedat::aedat31_decode_sequential(payload, n, o.source, f, c, put, &err))
                throw std::invalid_argument("aedat2bin: " + err + " (" + aedatFilePath + ")");
        } else {
            ecal_aedat::aedat20_decode_sequential(payload, n, f, c, put);
        }
        const auto dot = aedatFilePath.find_last_of('.');
        std::ofstream os(aedatFilePath.substr(0, dot) + ".bin", std::ofstream::binary | std::ofstream::trunc);
        os.write((const char *) out.data(), (std::streamsize) out.size());
        if (info)
            *info = ecal_aedat_info{c.n_raw_events, c.n_events, c.n_invalid, c.n_outside, c.n_negative, c.n_before_start, c.n_after_end,
                                    c.n_packets, c.n_other_packets, c.n_records, c.n_other_records, c.n_trailing_bytes, c.n_time_wraps,
                                    headerBytes, format};
        return (long long) c.n_events;
    }
    // aedat2bin on the device (ecal_aedat_to_bin_file: the packets indexed on the host, the payload uploaded and decoded in HBM): the
    // same arguments, the same output file name, the same bytes in it, the same returned count
    static long long aedat2binDevice(const std::string &aedatFilePath, const ecal_aedat_options *opt = nullptr, ecal_aedat_info *info = nullptr) {
        const auto dot = aedatFilePath.find_last_of('.');
        ecal_aedat_info I;
        ecal_ctx *ctx = ecal_host::thread_ctx();
        const int rc = ecal_aedat_to_bin_file(ctx, aedatFilePath.c_str(), (aedatFilePath.substr(0, dot) + ".bin").c_str(), opt, &I);
        if (rc == ECAL_ERR_INVALID) throw std::invalid_argument(std::string("aedat2binDevice: ") + ecal_last_error(ctx));
        if (rc != ECAL_OK) throw std::runtime_error(std::string("ecal_aedat_to_bin_file: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        if (info) *info = I;
        return (long long) I.n_events;
    }
    // An iniVation .aedat4 recording (DV: LZ4 packets of FlatBuffers; include/ecal.h, "aedat4 ingest") -> .bin beside it, on one host
    // thread: the plain sequential decoder of aedat4_events.hpp (header, chain, inflate, locate, filter), the records in file order.
    // The baseline of aedat42binDevice, and its check: both write the same bytes.  opt null: the defaults (the stream found by its
    // identifier, the automatic time base, no bounds, no flips).
    static long long aedat42bin(const std::string &aedat4FilePath, const ecal_aedat4_options *opt = nullptr, ecal_aedat4_info *info = nullptr) {
        std::ifstream is(aedat4FilePath, std::ifstream::binary);
        if (!is.is_open()) throw std::invalid_argument("No such file: " + aedat4FilePath);
        is.seekg(0, std::ifstream::end);
        std::vector<uint8_t> bytes((size_t) is.tellg());
        is.seekg(0);
        is.read((char *) bytes.data(), (std::streamsize) bytes.size());
        if ((size_t) is.gcount() != bytes.size()) throw std::runtime_error("aedat42bin: cannot read " + aedat4FilePath);
        ecal_aedat4_options o;
        if (opt) o = *opt; else ecal_aedat4_default_options(&o);
        if ((o.flip_x && !o.width) || (o.flip_y && !o.height)) throw std::invalid_argument("aedat42bin: flip_x / flip_y need width / height");
        const ecal_aedat4::A4DecodeOptions d{o.stream_id, o.auto_time_base,
                                             ecal_aedat4::A4Filter{o.time_base, o.width, o.height, o.start_time, o.has_end_time, o.end_time, o.flip_x, o.flip_y},
                                             o.max_inflated_bytes};
        ecal_aedat4::A4Counts c;
        std::vector<uint8_t> out;
        std::string err;
        auto put = [&](const uint8_t *rec) { out.insert(out.end(), rec, rec + Event::kRecordBytes); };
        static const uint8_t none = 0;
        const int rc = ecal_aedat4::a4_decode_sequential(bytes.empty() ? &none : bytes.data(), bytes.size(), d, c, put, &err);
        if (rc == ecal_aedat4::A4_INVALID) throw std::invalid_argument("aedat42bin: " + err + " (" + aedat4FilePath + ")");
        if (rc) throw std::runtime_error("aedat42bin: " + err + " (" + aedat4FilePath + ")");
        const auto dot = aedat4FilePath.find_last_of('.');
        std::ofstream os(aedat4FilePath.substr(0, dot) + ".bin", std::ofstream::binary | std::ofstream::trunc);
        os.write((const char *) out.data(), (std::streamsize) out.size());
        if (info)
            *info = ecal_aedat4_info{c.n_raw_events, c.n_events, c.n_outside, c.n_negative, c.n_before_start, c.n_after_end, c.n_packets,
                                     c.n_other_packets, c.n_trailing_bytes, c.n_compressed_bytes, c.n_inflated_bytes, c.first_stamp_us,
                                     c.time_base, c.compression, c.stream_id};
        return (long long) c.n_events;
    }
    // aedat42bin on the device (ecal_aedat4_to_bin_file: the packets indexed on the host, the file uploaded, inflated and decoded in
    // HBM): the same arguments, the same output file name, the same bytes in it, the same returned count
    static long long aedat42binDevice(const std::string &aedat4FilePath, const ecal_aedat4_options *opt = nullptr, ecal_aedat4_info *info = nullptr) {
        const auto dot = aedat4FilePath.find_last_of('.');
        ecal_aedat4_info I;
        ecal_ctx *ctx = ecal_host::thread_ctx();
        const int rc = ecal_aedat4_to_bin_file(ctx, aedat4FilePath.c_str(), (aedat4FilePath.substr(0, dot) + ".bin").c_str(), opt, &I);
        if (rc == ECAL_ERR_INVALID) throw std::invalid_argument(std::string("aedat42binDevice: ") + ecal_last_error(ctx));
        if (rc != ECAL_OK) throw std::runtime_error(std::string("ecal_aedat4_to_bin_file: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        if (info) *info = I;
        return (long long) I.n_events;
    }
    // A ROS 1 .bag of dvs_msgs/EventArray messages (format 2.0; include/ecal.h, "bag ingest") -> .bin beside it, on one host thread:
    // the plain sequential decoder of bag_events.hpp, the records in file order.  The baseline of bag2binDevice, and its check: both
    // write the same bytes.  opt null: the defaults (every connection of an event type, the automatic time base, no bounds, no flips).
    static long long bag2bin(const std::string &bagFilePath, const ecal_bag_options *opt = nullptr, ecal_bag_info *info = nullptr) {
        std::ifstream is(bagFilePath, std::ifstream::binary);
        if (!is.is_open()) throw std::invalid_argument("No such file: " + bagFilePath);
        is.seekg(0, std::ifstream::end);
        std::vector<uint8_t> bytes((size_t) is.tellg());
        is.seekg(0);
        is.read((char *) bytes.data(), (std::streamsize) bytes.size());
        if ((size_t) is.gcount() != bytes.size()) throw std::runtime_error("bag2bin: cannot read " + bagFilePath);
        ecal_bag_options o;
        if (opt) o = *opt; else ecal_bag_default_options(&o);
        if ((o.flip_x && !o.width) || (o.flip_y && !o.height)) throw std::invalid_argument("bag2bin: flip_x / flip_y need width / height");
        ecal_bag::BagChoice choice;
        if (o.topic) choice.topic = o.topic;
        if (o.type) choice.type = o.type;
        const ecal_bag::BagFilter f{o.time_base, o.width, o.height, o.start_time, o.has_end_time, o.end_time, o.flip_x, o.flip_y};
        ecal_bag::BagCounts c;
        std::vector<uint8_t> out;
        auto put = [&](const uint8_t *rec) { out.insert(out.end(), rec, rec + Event::kRecordBytes); };
        std::string err;
        int64_t base = 0;
        if (ecal_bag::bag_decode_sequential(bytes.data(), bytes.size(), choice, o.auto_time_base, f, c, put, &base, &err))
            throw std::invalid_argument("bag2bin: " + err + " (" + bagFilePath + ")");
        const auto dot = bagFilePath.find_last_of('.');
        std::ofstream os(bagFilePath.substr(0, dot) + ".bin", std::ofstream::binary | std::ofstream::trunc);
        os.write((const char *) out.data(), (std::streamsize) out.size());
        if (info)
            *info = ecal_bag_info{c.n_raw_events, c.n_events, c.n_outside, c.n_negative, c.n_before_start, c.n_after_end, c.n_messages,
                                  c.n_other_messages, c.n_chunks, c.n_connections, c.n_trailing_bytes, c.first_stamp_ns, base, c.msg_width,
                                  c.msg_height};
        return (long long) c.n_events;
    }
    // bag2bin on the device (ecal_bag_to_bin_file: the messages indexed on the host, the file uploaded and decoded in HBM): the same
    // arguments, the same output file name, the same bytes in it, the same returned count
    static long long bag2binDevice(const std::string &bagFilePath, const ecal_bag_options *opt = nullptr, ecal_bag_info *info = nullptr) {
        const auto dot = bagFilePath.find_last_of('.');
        ecal_bag_info I;
        ecal_ctx *ctx = ecal_host::thread_ctx();
        const int rc = ecal_bag_to_bin_file(ctx, bagFilePath.c_str(), (bagFilePath.substr(0, dot) + ".bin").c_str(), opt, &I);
        if (rc == ECAL_ERR_INVALID) throw std::invalid_argument(std::string("bag2binDevice: ") + ecal_last_error(ctx));
        if (rc != ECAL_OK) throw std::runtime_error(std::string("ecal_bag_to_bin_file: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        if (info) *info = I;
        return (long long) I.n_events;
    }
    // A ROS 2 .mcap recording of event messages (include/ecal_mcap.h) -> .bin beside it, on one host thread: the plain sequential
    // decoder of mcap_events.hpp, the records in file order.  The baseline of mcap2binDevice, and its check: both write the same bytes.
    // opt null: the defaults (every chosen channel, the automatic time base, no bounds, no flips).
    static long long mcap2bin(const std::string &mcapFilePath, const ecal_mcap_options *opt = nullptr, ecal_mcap_info *info = nullptr) {
        std::ifstream is(mcapFilePath, std::ifstream::binary);
        if (!is.is_open()) throw std::invalid_argument("No such file: " + mcapFilePath);
        is.seekg(0, std::ifstream::end);
        std::vector<uint8_t> bytes((size_t) is.tellg());
        is.seekg(0);
        is.read((char *) bytes.data(), (std::streamsize) bytes.size());
        if ((size_t) is.gcount() != bytes.size()) throw std::runtime_error("mcap2bin: cannot read " + mcapFilePath);
        ecal_mcap_options o;
        if (opt) o = *opt; else ecal_mcap_default_options(&o);
        if ((o.flip_x && !o.width) || (o.flip_y && !o.height)) throw std::invalid_argument("mcap2bin: flip_x / flip_y need width / height");
        const ecal_bag::BagFilter f{o.time_base, o.width, o.height, o.start_time, o.has_end_time, o.end_time, o.flip_x, o.flip_y};
        ecal_mcap::McapCounts c;
        std::vector<uint8_t> out;
        auto put = [&](const uint8_t *rec) { out.insert(out.end(), rec, rec + Event::kRecordBytes); };
        std::string err;
        int64_t base = 0;
        if (ecal_mcap::mcap_decode_sequential(bytes.data(), bytes.size(), o.topic ? o.topic : "", o.auto_time_base, f, c, put, &base, &err))
            throw std::invalid_argument("mcap2bin: " + err + " (" + mcapFilePath + ")");
        const auto dot = mcapFilePath.find_last_of('.');
        std::ofstream os(mcapFilePath.substr(0, dot) + ".bin", std::ofstream::binary | std::ofstream::trunc);
        os.write((const char *) out.data(), (std::streamsize) out.size());
        if (info) {
            ecal_mcap_info I;
            std::memset(&I, 0, sizeof(I));
            I.n_raw_events = c.n_raw_events; I.n_events = c.n_events; I.n_outside = c.n_outside; I.n_negative = c.n_negative;
            I.n_before_start = c.n_before_start; I.n_after_end = c.n_after_end; I.n_messages = c.n_messages;
            I.n_other_messages = c.n_other_messages; I.n_chunks = c.n_chunks; I.n_schemas = c.n_schemas; I.n_channels = c.n_channels;
            I.n_trailing_bytes = c.n_trailing_bytes; I.first_stamp_ns = c.first_stamp_ns; I.time_base = base; I.msg_width = c.msg_width;
            I.msg_height = c.msg_height; I.n_payload_bytes = c.n_payload_bytes; I.n_no_state = c.n_no_state;
            I.n_other_words = c.n_other_words; I.n_time_wraps = c.n_time_wraps;
            std::memcpy(&I.layout, &c.layout, sizeof(I.layout));
            *info = I;
        }
        return (long long) c.n_events;
    }
    // mcap2bin on the device (ecal_mcap_to_bin_file: the messages indexed on the host, the file uploaded and decoded in HBM): the same
    // arguments, the same output file name, the same bytes in it, the same returned count
    static long long mcap2binDevice(const std::string &mcapFilePath, const ecal_mcap_options *opt = nullptr, ecal_mcap_info *info = nullptr) {
        const auto dot = mcapFilePath.find_last_of('.');
        ecal_mcap_info I;
        ecal_ctx *ctx = ecal_host::thread_ctx();
        const int rc = ecal_mcap_to_bin_file(ctx, mcapFilePath.c_str(), (mcapFilePath.substr(0, dot) + ".bin").c_str(), opt, &I);
        if (rc == ECAL_ERR_INVALID) throw std::invalid_argument(std::string("mcap2binDevice: ") + ecal_last_error(ctx));
        if (rc != ECAL_OK) throw std::runtime_error(std::string("ecal_mcap_to_bin_file: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        if (info) *info = I;
        return (long long) I.n_events;
    }
    // A .npy file of events (a 1-D structured array or an (N, 4) array; include/ecal.h, "array ingest") -> .bin beside it, on one host
    // thread: the header parser and the plain walk of fields_events.hpp, the records in file order.  The baseline of npy2binDevice,
    // and its check: both write the same bytes.  opt null: the defaults (1e-6 s a tick, base 0, no bounds, no flips).
    static long long npy2bin(const std::string &npyFilePath, const ecal_npy_options *opt = nullptr, ecal_fields_info *info = nullptr) {
        std::ifstream is(npyFilePath, std::ifstream::binary);
        if (!is.is_open()) throw std::invalid_argument("No such file: " + npyFilePath);
        is.seekg(0, std::ifstream::end);
        std::vector<uint8_t> bytes((size_t) is.tellg());
        is.seekg(0);
        is.read((char *) bytes.data(), (std::streamsize) bytes.size());
        if ((size_t) is.gcount() != bytes.size()) throw std::runtime_error("npy2bin: cannot read " + npyFilePath);
        ecal_npy_options o;
        if (opt) o = *opt; else ecal_npy_default_options(&o);
        ecal_fields::NpyChoice choice;
        const char *names[4] = {o.t_name, o.x_name, o.y_name, o.p_name};
        for (int k = 0; k < 4; k++)
            if (names[k]) choice.name[k] = names[k];
        if (o.columns) choice.columns = o.columns;
        ecal_fields::NpyLayout L;
        std::string err;
        if (ecal_fields::npy_parse_header(bytes.data(), bytes.size(), 0, choice, L, &err))
            throw std::invalid_argument("npy2bin: " + err + " (" + npyFilePath + ")");
        ecal_fields::Field f[4];
        for (int k = 0; k < 4; k++) f[k] = ecal_fields::Field{bytes.data() + L.data_offset + L.field[k].offset, (int64_t) L.item_stride, L.field[k].type, 0u};
        if (o.fields.auto_time_base) o.fields.time_base = ecal_fields::fd_auto_time_base(f[0], L.n_events);
        const ecal_fields::FieldsFilter flt{o.fields.time_magnitude, o.fields.time_base, o.fields.width, o.fields.height, o.fields.start_time,
                                            o.fields.has_end_time, o.fields.end_time, o.fields.flip_x, o.fields.flip_y};
        if (ecal_fields::fd_check_filter(flt, f[0].type, &err)) throw std::invalid_argument("npy2bin: " + err);
        ecal_fields::FieldsCounts c;
        std::vector<uint8_t> out;
        ecal_fields::fd_walk(f, L.n_events, flt, c, [&](const uint8_t *rec) { out.insert(out.end(), rec, rec + Event::kRecordBytes); });
        const auto dot = npyFilePath.find_last_of('.');
        std::ofstream os(npyFilePath.substr(0, dot) + ".bin", std::ofstream::binary | std::ofstream::trunc);
        os.write((const char *) out.data(), (std::streamsize) out.size());
        if (info) *info = ecal_fields_info{c.n_raw_events, c.n_events, c.n_outside, c.n_negative, c.n_before_start, c.n_after_end, flt.time_base};
        return (long long) c.n_events;
    }
    // npy2bin on the device (ecal_npy_to_bin_file: the header on the host, the payload uploaded and decoded in HBM): the same
    // arguments, the same output file name, the same bytes in it, the same returned count
    static long long npy2binDevice(const std::string &npyFilePath, const ecal_npy_options *opt = nullptr, ecal_fields_info *info = nullptr) {
        const auto dot = npyFilePath.find_last_of('.');
        ecal_fields_info I;
        ecal_ctx *ctx = ecal_host::thread_ctx();
        const int rc = ecal_npy_to_bin_file(ctx, npyFilePath.c_str(), (npyFilePath.substr(0, dot) + ".bin").c_str(), opt, &I);
        if (rc == ECAL_ERR_INVALID) throw std::invalid_argument(std::string("npy2binDevice: ") + ecal_last_error(ctx));
        if (rc != ECAL_OK) throw std::runtime_error(std::string("ecal_npy_to_bin_file: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        if (info) *info = I;
        return (long long) I.n_events;
    }
    // txt2bin's arguments as ecal_text_options (LLONG_MIN: no base / no end, as there)
    static ecal_text_options textOptions(double timeMagnitude, long long timeBase_in, long long endTime_in) {
        ecal_text_options opt;
        ecal_text_default_options(&opt);
        opt.time_magnitude = timeMagnitude;
        opt.has_time_base = timeBase_in != std::numeric_limits<long long>::min();
        opt.time_base = opt.has_time_base ? timeBase_in : 0;
        opt.has_end_stamp = endTime_in != std::numeric_limits<long long>::min();
        opt.end_stamp = opt.has_end_stamp ? endTime_in : 0;
        return opt;
    }

private:
    void advance() {
        is_.read((char *) rec_, Event::kRecordBytes);
        if (is_.gcount() != (std::streamsize) Event::kRecordBytes) {
            end_ = true;
            return;
        }
        cur_ = Event::unpack(rec_);
    }
    std::ifstream is_;
    Event cur_;
    uint8_t rec_[Event::kRecordBytes];
    bool end_ = false;
};

// The reference keeps a std::multimap<double, Event_loc_pol> on the host; here the time-ordered
// records live in HBM (one upload), and frames are cut out of them on the GPU.
struct EventContainer {
    typedef std::shared_ptr<EventContainer> Ptr;

    void emplace(const Event &e) {  // append in time order (the file order of a .bin)
        uint8_t r[Event::kRecordBytes];
        const double t = e.timeStamp();
        std::memcpy(r, &t, 8);
        std::memcpy(r + 8, &e.location()[0], 8);
        std::memcpy(r + 16, &e.location()[1], 8);
        r[24] = e.polarity() ? 1 : 0;
        if (fromFile_) throw std::logic_error("EventContainer: emplace after loadFile (the records live in HBM only)");
        records.insert(records.end(), r, r + Event::kRecordBytes);
        if (stream_) release();
    }
    // The whole reading loop of eventCameraCalib.cpp:154-163 in one call (ecal_stream_create_from_file): the records with
    // timeStamp >= startTime — up to the first one with timeStamp >= endTime when customEnd — go from the file straight
    // to HBM (chunked reads overlapped with the upload); `records` stays empty.
    void loadFile(const std::string &binFilePath, double startTime, bool customEnd = false, double endTime = 0.0) {
        release();
        records.clear();
        const int rc = ecal_stream_create_from_file(ecal_host::thread_ctx(), binFilePath.c_str(), startTime, customEnd ? 1 : 0, endTime,
                                                    &stream_);
        if (rc == ECAL_ERR_INVALID) throw std::invalid_argument("No such file: " + binFilePath);
        if (rc != ECAL_OK)
            throw std::runtime_error(std::string("ecal_stream_create_from_file: ") + ecal_strerror(rc) + " — " +
                                     ecal_last_error(ecal_host::thread_ctx()));
        if (ecal_stream_times(stream_, &devFirst_, &devLast_) != ECAL_OK) throw std::runtime_error("ecal_stream_times");
        fromFile_ = true;
    }
    // The same from a text file of "stamp x y polarity" lines (ecal_stream_create_from_text_file): txt2bin's conversion
    // (timeMagnitude, timeBase_in, endTime_in as EventStream::txt2bin takes them) and the reading loop above in one pass on the
    // device, without the .bin in between.
    void loadTextFile(const std::string &txtFilePath, double timeMagnitude = 1e-6,
                      long long timeBase_in = std::numeric_limits<long long>::min(),
                      long long endTime_in = std::numeric_limits<long long>::min(),
                      double startTime = -std::numeric_limits<double>::infinity(), bool customEnd = false, double endTime = 0.0) {
        release();
        records.clear();
        ecal_text_options opt = EventStream::textOptions(timeMagnitude, timeBase_in, endTime_in);
        opt.start_time = startTime;
        opt.has_end_time = customEnd ? 1 : 0;
        opt.end_time = endTime;
        ecal_ctx *ctx = ecal_host::thread_ctx();
        const int rc = ecal_stream_create_from_text_file(ctx, txtFilePath.c_str(), &opt, &stream_, &textInfo);
        if (rc == ECAL_ERR_INVALID) throw std::invalid_argument(std::string("loadTextFile: ") + ecal_last_error(ctx));
        if (rc != ECAL_OK)
            throw std::runtime_error(std::string("ecal_stream_create_from_text_file: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        if (ecal_stream_times(stream_, &devFirst_, &devLast_) != ECAL_OK) throw std::runtime_error("ecal_stream_times");
        fromFile_ = true;
    }
    ecal_text_info textInfo{};   // what the last loadTextFile saw (lines, drops, host-parsed lines)
    // The same from a Prophesee .raw recording (ecal_stream_create_from_raw_file): decoded on the device, without a .bin in
    // between.  opt null: the defaults; the reading loop's startTime / customEnd / endTime go into opt's start_time / end_time.
    void loadRawFile(const std::string &rawFilePath, const ecal_raw_options *opt = nullptr) {
        release();
        records.clear();
        ecal_ctx *ctx = ecal_host::thread_ctx();
        const int rc = ecal_stream_create_from_raw_file(ctx, rawFilePath.c_str(), opt, &stream_, &rawInfo);
        if (rc == ECAL_ERR_INVALID) throw std::invalid_argument(std::string("loadRawFile: ") + ecal_last_error(ctx));
        if (rc != ECAL_OK)
            throw std::runtime_error(std::string("ecal_stream_create_from_raw_file: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        if (ecal_stream_times(stream_, &devFirst_, &devLast_) != ECAL_OK) throw std::runtime_error("ecal_stream_times");
        fromFile_ = true;
    }
    ecal_raw_info rawInfo{};     // what the last loadRawFile saw (words, drops, wraps, the format in force)
    // The same from an iniVation .aedat recording (ecal_stream_create_from_aedat_file): decoded on the device, without a .bin in
    // between.  opt null: the defaults; the reading loop's startTime / customEnd / endTime go into opt's start_time / end_time.
    void loadAedatFile(const std::string &aedatFilePath, const ecal_aedat_options *opt = nullptr) {
        release();
        records.clear();
        ecal_ctx *ctx = ecal_host::thread_ctx();
        const int rc = ecal_stream_create_from_aedat_file(ctx, aedatFilePath.c_str(), opt, &stream_, &aedatInfo);
        if (rc == ECAL_ERR_INVALID) throw std::invalid_argument(std::string("loadAedatFile: ") + ecal_last_error(ctx));
        if (rc != ECAL_OK)
            throw std::runtime_error(std::string("ecal_stream_create_from_aedat_file: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        if (ecal_stream_times(stream_, &devFirst_, &devLast_) != ECAL_OK) throw std::runtime_error("ecal_stream_times");
        fromFile_ = true;
    }
    ecal_aedat_info aedatInfo{}; // what the last loadAedatFile saw (packets, records, drops, wraps, the format in force)
    // The same from an iniVation .aedat4 recording (ecal_stream_create_from_aedat4_file): inflated and decoded on the device.
    void loadAedat4File(const std::string &aedat4FilePath, const ecal_aedat4_options *opt = nullptr) {
        release();
        records.clear();
        ecal_ctx *ctx = ecal_host::thread_ctx();
        const int rc = ecal_stream_create_from_aedat4_file(ctx, aedat4FilePath.c_str(), opt, &stream_, &aedat4Info);
        if (rc == ECAL_ERR_INVALID) throw std::invalid_argument(std::string("loadAedat4File: ") + ecal_last_error(ctx));
        if (rc != ECAL_OK)
            throw std::runtime_error(std::string("ecal_stream_create_from_aedat4_file: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        if (ecal_stream_times(stream_, &devFirst_, &devLast_) != ECAL_OK) throw std::runtime_error("ecal_stream_times");
        fromFile_ = true;
    }
    ecal_aedat4_info aedat4Info{}; // what the last loadAedat4File saw (packets, bytes, drops, the stream and the time base in force)
    // The same from a ROS 1 .bag of event arrays (ecal_stream_create_from_bag_file): decoded on the device, without a .bin in between.
    // opt null: the defaults; the reading loop's startTime / customEnd / endTime go into opt's start_time / end_time.
    void loadBagFile(const std::string &bagFilePath, const ecal_bag_options *opt = nullptr) {
        release();
        records.clear();
        ecal_ctx *ctx = ecal_host::thread_ctx();
        const int rc = ecal_stream_create_from_bag_file(ctx, bagFilePath.c_str(), opt, &stream_, &bagInfo);
        if (rc == ECAL_ERR_INVALID) throw std::invalid_argument(std::string("loadBagFile: ") + ecal_last_error(ctx));
        if (rc != ECAL_OK)
            throw std::runtime_error(std::string("ecal_stream_create_from_bag_file: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        if (ecal_stream_times(stream_, &devFirst_, &devLast_) != ECAL_OK) throw std::runtime_error("ecal_stream_times");
        fromFile_ = true;
    }
    ecal_bag_info bagInfo{};     // what the last loadBagFile saw (messages, chunks, drops, the time base in force)
    // The same from a ROS 2 .mcap recording of event messages (ecal_stream_create_from_mcap_file, include/ecal_mcap.h).
    void loadMcapFile(const std::string &mcapFilePath, const ecal_mcap_options *opt = nullptr) {
        release();
        records.clear();
        ecal_ctx *ctx = ecal_host::thread_ctx();
        const int rc = ecal_stream_create_from_mcap_file(ctx, mcapFilePath.c_str(), opt, &stream_, &mcapInfo);
        if (rc == ECAL_ERR_INVALID) throw std::invalid_argument(std::string("loadMcapFile: ") + ecal_last_error(ctx));
        if (rc != ECAL_OK)
            throw std::runtime_error(std::string("ecal_stream_create_from_mcap_file: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        if (ecal_stream_times(stream_, &devFirst_, &devLast_) != ECAL_OK) throw std::runtime_error("ecal_stream_times");
        fromFile_ = true;
    }
    ecal_mcap_info mcapInfo{};   // what the last loadMcapFile saw (messages, chunks, drops, the kind, the layout and the time base in force)
    // The same from events held as four columns in host memory (ecal_stream_create_from_fields: f[4] = t, x, y, p, element i at
    // ptr + i * stride, any of the nine ECAL_FIELD_* types): uploaded as they lie and packed on the device.  opt null: the defaults.
    void loadArrays(const ecal_field f[4], uint64_t n, const ecal_fields_options *opt = nullptr) {
        release();
        records.clear();
        ecal_ctx *ctx = ecal_host::thread_ctx();
        const int rc = ecal_stream_create_from_fields(ctx, f, n, opt, &stream_, &fieldsInfo);
        if (rc == ECAL_ERR_INVALID) throw std::invalid_argument(std::string("loadArrays: ") + ecal_last_error(ctx));
        if (rc != ECAL_OK)
            throw std::runtime_error(std::string("ecal_stream_create_from_fields: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        if (ecal_stream_times(stream_, &devFirst_, &devLast_) != ECAL_OK) throw std::runtime_error("ecal_stream_times");
        fromFile_ = true;
    }
    // ... and from a .npy file of events (ecal_stream_create_from_npy_file): the header on the host, the payload decoded on the device.
    void loadNpyFile(const std::string &npyFilePath, const ecal_npy_options *opt = nullptr) {
        release();
        records.clear();
        ecal_ctx *ctx = ecal_host::thread_ctx();
        const int rc = ecal_stream_create_from_npy_file(ctx, npyFilePath.c_str(), opt, &stream_, &fieldsInfo);
        if (rc == ECAL_ERR_INVALID) throw std::invalid_argument(std::string("loadNpyFile: ") + ecal_last_error(ctx));
        if (rc != ECAL_OK)
            throw std::runtime_error(std::string("ecal_stream_create_from_npy_file: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        if (ecal_stream_times(stream_, &devFirst_, &devLast_) != ECAL_OK) throw std::runtime_error("ecal_stream_times");
        fromFile_ = true;
    }
    ecal_fields_info fieldsInfo{};   // what the last loadArrays / loadNpyFile saw (drops, the time base in force)
    // The events of hot pixels taken out of a file-backed container (ecal_stream_remove_hot_pixels: a per-pixel count, the rule, an
    // order-preserving filter; opt null: the defaults on a 346 x 260 sensor): the stream is swapped for the filtered one.
    // firstTime() / lastTime() stay the loaded stream's.  maskOut [height * width] / countsOut [2][height][width]: may be null.
    void removeHotPixels(const ecal_hot_pixel_options *opt = nullptr, ecal_hot_pixel_info *info = nullptr, uint8_t *maskOut = nullptr,
                         uint32_t *countsOut = nullptr) {
        if (!fromFile_ || !stream_) throw std::logic_error("EventContainer: removeHotPixels needs a file-backed container (loadFile and its kin)");
        ecal_ctx *ctx = ecal_host::thread_ctx();
        ecal_stream *filtered = nullptr;
        const int rc = ecal_stream_remove_hot_pixels(ctx, stream_, opt, nullptr, &filtered, maskOut, countsOut, &hotPixelInfo);
        if (info) *info = hotPixelInfo;
        if (rc == ECAL_ERR_INVALID) throw std::invalid_argument(std::string("removeHotPixels: ") + ecal_last_error(ctx));
        if (rc != ECAL_OK)
            throw std::runtime_error(std::string("ecal_stream_remove_hot_pixels: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        ecal_stream_destroy(stream_);
        stream_ = filtered;
    }
    ecal_hot_pixel_info hotPixelInfo{};   // what the last removeHotPixels saw (events and pixels, removed and kept)
    // The events without a recent neighbour event taken out of a file-backed container (ecal_stream_remove_noise: every event judged
    // on the device from the stream alone, an order-preserving filter; opt null: the defaults on a 346 x 260 sensor): the stream is
    // swapped for the filtered one.  firstTime() / lastTime() stay the loaded stream's.  Hot pixels first when both are wanted.
    void removeNoise(const ecal_noise_options *opt = nullptr, ecal_filter_totals *totals = nullptr) {
        if (!fromFile_ || !stream_) throw std::logic_error("EventContainer: removeNoise needs a file-backed container (loadFile and its kin)");
        ecal_ctx *ctx = ecal_host::thread_ctx();
        ecal_stream *filtered = nullptr;
        const int rc = ecal_stream_remove_noise(ctx, stream_, opt, &filtered, &noiseTotals);
        if (totals) *totals = noiseTotals;
        if (rc == ECAL_ERR_INVALID) throw std::invalid_argument(std::string("removeNoise: ") + ecal_last_error(ctx));
        if (rc != ECAL_OK) throw std::runtime_error(std::string("ecal_stream_remove_noise: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        ecal_stream_destroy(stream_);
        stream_ = filtered;
    }
    ecal_filter_totals noiseTotals{};     // what the last removeNoise saw (events, off the grid, removed, kept)
    // The events as the ideal pinhole camera behind `camera` (the solved intrinsics: ecal_undistort_camera_from_params) would have seen
    // them, as a container of its own (ecal_stream_undistort; this one is untouched): invalid events are gone, in PIXEL mode those
    // outside the canvas too; stamps, polarities and the order stay.  opt null: sub-pixel coordinates.
    Ptr undistorted(const ecal_undistort_camera &camera, const ecal_undistort_options *opt = nullptr, ecal_undistort_totals *totals = nullptr) {
        ecal_ctx *ctx = ecal_host::thread_ctx();
        Ptr out = std::make_shared<EventContainer>();
        out->cameraSize = cameraSize;
        const int rc = ecal_stream_undistort(ctx, device(), &camera, opt, &out->stream_, &undistortTotals);
        if (totals) *totals = undistortTotals;
        if (rc == ECAL_ERR_INVALID) throw std::invalid_argument(std::string("undistorted: ") + ecal_last_error(ctx));
        if (rc != ECAL_OK) throw std::runtime_error(std::string("ecal_stream_undistort: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        out->fromFile_ = true;
        if (ecal_stream_size(out->stream_) && ecal_stream_times(out->stream_, &out->devFirst_, &out->devLast_) != ECAL_OK)
            throw std::runtime_error("ecal_stream_times");
        return out;
    }
    ecal_undistort_totals undistortTotals{};   // what the last undistorted saw (events, invalid, outside, kept)
    size_t size() const { return fromFile_ ? (size_t) ecal_stream_size(stream_) : records.size() / Event::kRecordBytes; }
    double firstTime() const { return fromFile_ ? devFirst_ : Event::unpack(records.data()).timeStamp(); }
    double lastTime() const {
        return fromFile_ ? devLast_ : Event::unpack(records.data() + records.size() - Event::kRecordBytes).timeStamp();
    }

    // device image, uploaded lazily; throws if the records are not in time order
    const ecal_stream *device() {
        if (!stream_) {
            const int rc = ecal_stream_create(ecal_host::thread_ctx(), records.data(), size(), &stream_);
            if (rc != ECAL_OK)
                throw std::runtime_error(std::string("ecal_stream_create: ") + ecal_strerror(rc) + " — " +
                                         ecal_last_error(ecal_host::thread_ctx()));
        }
        return stream_;
    }
    void release() {
        if (stream_) ecal_stream_destroy(stream_);
        stream_ = nullptr;
        fromFile_ = false;
    }
    ~EventContainer() { release(); }

    std::vector<uint8_t> records;  // packed 25-byte records
    Vector2d cameraSize{{346, 260}};  // (width, height) of the sensor (CameraBase::size())

private:
    ecal_stream *stream_ = nullptr;
    bool fromFile_ = false;
    double devFirst_ = 0, devLast_ = 0;
};

// Result of the GPU pass over one window (shared by EventFrame and CirclesEventFrame)
struct FrameDetection {
    std::vector<Vector2d> positive, negative;  // positiveEvents_ / negativeEvents_, canonical order
    std::vector<int32_t> labelsPos, labelsNeg;  // DBSCAN labels (index into Clusters, -1 = Noise)
    std::vector<int32_t> keptPos, keptNeg;      // after the clusterMinSample filter
    uint32_t nClustersPos = 0, nClustersNeg = 0, keptClustersPos = 0, keptClustersNeg = 0, status = 1;
    bool tieFallback = false;   // ECAL_WIN_TIE_FALLBACK: a tied median of this window is not guaranteed to be the reference's pick
    std::vector<std::pair<size_t, size_t>> candidates;  // (+ cluster, - cluster), kept numbering
    std::vector<Vector2d> candidateCenters;
    std::vector<double> candidatesRadius;
    bool gridFound = false;            // cv::findCirclesGrid's isFound (CirclesEventFrame.cpp:332-336)
    std::vector<size_t> orderIdxs;     // candidate index per grid position i*cols + j (:343-348)
};

inline void detect_windows(EventContainer &c, const std::vector<std::pair<double, double>> &durations,
                           const ecal_detect_params &prm, std::vector<FrameDetection> &out) {
    const uint32_t S = (uint32_t) durations.size();
    out.assign(S, FrameDetection());
    if (S == 0) return;
    std::vector<double> t0(S), t1(S);
    for (uint32_t s = 0; s < S; s++) {
        t0[s] = durations[s].first;
        t1[s] = durations[s].second;
    }
    ecal_ctx *ctx = ecal_host::thread_ctx();
    // capacity: windows may overlap, so count the covered events first (bounds only, cheap)
    std::vector<uint32_t> base(S + 1);
    ecal_detect_result probe;
    std::memset(&probe, 0, sizeof(probe));
    probe.win_base = base.data();
    size_t cap = c.size();
    std::vector<double> xy;
    const uint32_t M = prm.rows * prm.cols;
    std::vector<int32_t> gorder((size_t) S * (M ? M : 1));
    std::vector<uint32_t> gfound(S, 0);
    std::vector<uint32_t> seg_off(2 * S), seg_cnt(2 * S), ncl(2 * S), info(4 * S), pair;
    std::vector<int32_t> labels, kept;
    std::vector<double> xyr;
    for (int attempt = 0; attempt < 2; attempt++) {
        xy.resize(2 * cap);
        labels.resize(cap);
        kept.resize(cap);
        pair.resize(2 * cap);
        xyr.resize(3 * cap);
        ecal_detect_result r;
        std::memset(&r, 0, sizeof(r));
        r.win_base = base.data();
        r.xy = xy.data();
        r.seg_off = seg_off.data();
        r.seg_cnt = seg_cnt.data();
        r.labels = labels.data();
        r.n_clusters = ncl.data();
        r.kept_labels = kept.data();
        r.win_info = info.data();
        r.cand_pair = pair.data();
        r.cand_xyr = xyr.data();
        r.grid_order = gorder.data();
        r.grid_found = gfound.data();
        const int rc = ecal_detect_batch(ctx, c.device(), t0.data(), t1.data(), S, &prm, (uint32_t) cap, &r);
        if (rc == ECAL_OK) break;
        if (rc == ECAL_ERR_RANGE && attempt == 0) {  // overlapping windows cover more slots than events
            cap = (size_t) base[S] + 16;
            continue;
        }
        throw std::runtime_error(std::string("ecal_detect_batch: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
    }
    for (uint32_t s = 0; s < S; s++) {
        FrameDetection &f = out[s];
        const uint32_t op = seg_off[2 * s], np = seg_cnt[2 * s], on = seg_off[2 * s + 1], nn = seg_cnt[2 * s + 1];
        f.positive.resize(np);
        f.negative.resize(nn);
        for (uint32_t i = 0; i < np; i++) f.positive[i] = Vector2d{{xy[2 * (op + i)], xy[2 * (op + i) + 1]}};
        for (uint32_t i = 0; i < nn; i++) f.negative[i] = Vector2d{{xy[2 * (on + i)], xy[2 * (on + i) + 1]}};
        f.labelsPos.assign(labels.begin() + op, labels.begin() + op + np);
        f.labelsNeg.assign(labels.begin() + on, labels.begin() + on + nn);
        f.keptPos.assign(kept.begin() + op, kept.begin() + op + np);
        f.keptNeg.assign(kept.begin() + on, kept.begin() + on + nn);
        f.nClustersPos = ncl[2 * s];
        f.nClustersNeg = ncl[2 * s + 1];
        f.keptClustersPos = info[4 * s + 1];
        f.keptClustersNeg = info[4 * s + 2];
        f.status = ECAL_WIN_STATUS(info[4 * s + 3]);
        f.tieFallback = (info[4 * s + 3] & ECAL_WIN_TIE_FALLBACK) != 0;
        for (uint32_t j = 0; j < info[4 * s]; j++) {
            f.candidates.emplace_back(pair[2 * (op + j)], pair[2 * (op + j) + 1]);
            f.candidateCenters.push_back(Vector2d{{xyr[3 * (op + j)], xyr[3 * (op + j) + 1]}});
            f.candidatesRadius.push_back(xyr[3 * (op + j) + 2]);
        }
        f.gridFound = M > 0 && gfound[s] != 0;
        if (f.gridFound)
            for (uint32_t m = 0; m < M; m++) f.orderIdxs.push_back((size_t) gorder[(size_t) s * M + m]);
    }
}

// EventFrame: events with duration.first <= t <= duration.second, per-polarity unique pixel sets,
// pixels that fired with both polarities removed (EventFrame.cpp:10-36).
class EventFrame {
public:
    EventFrame(EventContainer::Ptr container, const std::pair<double, double> &duration)
        : container_(std::move(container)), duration_(duration) {}
    virtual ~EventFrame() {}
    int eventsNum() {
        ensure();
        return (int) (det_.positive.size() + det_.negative.size());
    }
    void releaseEventSet() {
        det_.positive.clear();
        det_.negative.clear();
    }
    const std::vector<Vector2d> &positiveEvents() {
        ensure();
        return det_.positive;
    }
    const std::vector<Vector2d> &negativeEvents() {
        ensure();
        return det_.negative;
    }
    // EventFrame::undistortedImage (EventFrame.cpp:38-60) for the camera's size of the container: the RGB bytes of the canvas
    // round(1.2 * size) — ecal_undistort_reference_canvas; width and height through the pointers —, red where a positive point of
    // the frame lands, green where a negative one does (painted over the red).  Points that are invalid or land outside the canvas
    // are painted nowhere (the reference indexes out of bounds there).
    std::vector<uint8_t> undistortedImage(const ecal_undistort_camera &camera, int *widthOut = nullptr, int *heightOut = nullptr,
                                          ecal_undistort_frame_totals *totals = nullptr) {
        ensure();
        if (det_.positive.empty() || det_.negative.empty()) throw std::logic_error("Events in Frame was cleared.");
        ecal_undistort_options opt;
        ecal_undistort_reference_canvas((uint32_t) container_->cameraSize[0], (uint32_t) container_->cameraSize[1], &opt);
        std::vector<uint8_t> rgb((size_t) opt.out_width * opt.out_height * 3);
        ecal_ctx *ctx = ecal_host::thread_ctx();
        const int rc = ecal_stream_undistorted_frames(ctx, container_->device(), &camera, &opt, &duration_.first, &duration_.second, 1, rgb.data(),
                                                      totals);
        if (rc == ECAL_ERR_INVALID) throw std::invalid_argument(std::string("undistortedImage: ") + ecal_last_error(ctx));
        if (rc != ECAL_OK)
            throw std::runtime_error(std::string("ecal_stream_undistorted_frames: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        if (widthOut) *widthOut = (int) opt.out_width;
        if (heightOut) *heightOut = (int) opt.out_height;
        return rgb;
    }

protected:
    virtual ecal_detect_params params() const {
        ecal_detect_params p;
        p.dbscan_eps = 4;
        p.dbscan_min_samples = 2;
        p.cluster_min_sample = 5;
        p.need_clusters = 36;
        p.circle_radius_threshold = ecal_circle_radius_threshold(346, 260, 9, 4, 1, 5.5, 1.75);
        p.fit_circle = 0;
        p.knn_num = 3;
        p.rows = 0;
        p.cols = 0;
        return p;
    }
    void ensure() {
        if (done_) return;
        std::vector<FrameDetection> out;
        detect_windows(*container_, {duration_}, params(), out);
        det_ = std::move(out[0]);
        done_ = true;
    }
    EventContainer::Ptr container_;
    std::pair<double, double> duration_;
    FrameDetection det_;
    bool done_ = false;
};

}  // namespace opengv2

#endif  // ECAL_HOST_EVENT_HPP_
