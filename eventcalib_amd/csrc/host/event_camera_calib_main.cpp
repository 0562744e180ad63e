// unit_test_eventCameraCalib: the reference driver's main (event_camera_calib/test/eventCameraCalib.cpp:99-233) on the C++ shims:
// stream -> container -> keyframe search -> EventCalibIni::cvCalibration (+ rectifyFeatures per keyframe) ->
// EventCalibSpline -> TrajectoryByEvent.txt.  Built by eventcalib_amd/csrc/Makefile (`make driver`, part of `all`) into
// eventcalib_amd/unit_test_eventCameraCalib next to libecal.so; run by tests/test_gpu_shims.py and bench.py's end_to_end leg.
//   usage: unit_test_eventCameraCalib settings.yaml events.bin saveDir [batch]     (the reference's argv, eventCameraCalib.cpp:105-110;
//   with batch, an events path ending in .txt is a text file of "stamp x y polarity" lines, converted on the device; one ending in
//   .raw, .aedat, .aedat4, .bag or .mcap a camera's or recorder's own file, .npy events as numpy saves them, decoded on the device)
// "batch": rectifyFeatures of all keyframes in one device pass (ecal_rectify_keyframes) instead of one CirclesEventFrame per
// keyframe, the file read in one piece, and a "stage <name> <seconds>" line per stage of the chain (bench.py's end_to_end leg).
#include <chrono>
#include <cstdio>

#include <filesystem>
#include <thread>
#include <algorithm>

#include "event_calib_spline.hpp"
#include "png_writer.hpp"
#include "npy_writer.hpp"
#include "pinhole_camera.hpp"

int main(int argc, char **argv) {
    using namespace opengv2;
    const bool batch = argc == 5 && std::string(argv[4]) == "batch";
    double t_mark = 0;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    auto stage = [&](const char *name) {
        const double t = now();
        if (batch) std::printf("stage %s %.6f\n", name, t - t_mark);
        t_mark = t;
    };
    t_mark = now();
    if (argc != 4 && !batch) {
        std::fprintf(stderr, "Usage: unit_test_eventCameraCalib settingFilePath binFilePath SavePath\n");
        return 1;
    }
    FileSettings fsSettings(argv[1]);                        // :114-118
    if (!fsSettings.isOpened()) {
        std::fprintf(stderr, "Failed to open settings file at: %s\n", argv[1]);
        return 2;
    }
    auto cs = std::make_shared<CalibrationSetting>(fsSettings);   // :121
    const double step = fsSettings["MotionTimeStep"];        // :126
    const bool customEnd = !fsSettings["EndTime"].isNone();  // :150-153
    const double startTime = fsSettings["StartTime"];
    const double endTimeSetting = customEnd ? (double) fsSettings["EndTime"] : 0.0;
    EventStream es(argv[2]);
    auto container = std::make_shared<EventContainer>();
    int width = fsSettings["Camera.width"], height = fsSettings["Camera.height"];   // :141-142
    container->cameraSize[0] = width;
    container->cameraSize[1] = height;
    if (batch) {   // the same loop as one call: file -> HBM, reads and upload overlapped (EventContainer::loadFile)
        (void) ecal_host::thread_ctx();   // HIP runtime + context start-up (0.2 - 0.3 s in a cold process): a stage of its own,
        stage("runtime_init");            // not part of reading the file
        es.close();
        const std::string eventsPath = argv[2];
        if (eventsPath.size() >= 4 && eventsPath.compare(eventsPath.size() - 4, 4, ".txt") == 0) {
            // a text file of "stamp x y polarity" lines: txt2bin's conversion and the loop below in one device pass.  Keys of this
            // build, both optional: Text_TimeMagnitude (seconds per stamp unit, 1e-6), Text_TimeBase (absent: the first stamp)
            double magnitude = 1e-6;
            fsSettings["Text_TimeMagnitude"] >> magnitude;
            long long timeBase = std::numeric_limits<long long>::min();
            if (!fsSettings["Text_TimeBase"].isNone()) timeBase = std::strtoll(((std::string) fsSettings["Text_TimeBase"]).c_str(), nullptr, 10);
            container->loadTextFile(eventsPath, magnitude, timeBase, std::numeric_limits<long long>::min(), startTime, customEnd, endTimeSetting);
        } else if (eventsPath.size() >= 4 && eventsPath.compare(eventsPath.size() - 4, 4, ".raw") == 0) {
            // a Prophesee recording (EVT3 / EVT2) decoded on the device.  Keys of this build, both optional: Raw_Format ("EVT2" /
            // "EVT3"; absent: from the file's header), Raw_TimeBase (microseconds of the camera's clock, 0).  Events outside
            // Camera.width x Camera.height are dropped.
            ecal_raw_options opt;
            ecal_raw_default_options(&opt);
            if (!fsSettings["Raw_Format"].isNone()) {
                const std::string fmt = fsSettings["Raw_Format"];
                opt.format = fmt == "EVT2" ? ECAL_RAW_EVT2 : fmt == "EVT3" ? ECAL_RAW_EVT3 : -1;   // (-1: refused by the library)
            }
            if (!fsSettings["Raw_TimeBase"].isNone()) opt.time_base = std::strtoll(((std::string) fsSettings["Raw_TimeBase"]).c_str(), nullptr, 10);
            opt.width = (uint32_t) width;
            opt.height = (uint32_t) height;
            opt.start_time = startTime;
            opt.has_end_time = customEnd ? 1 : 0;
            opt.end_time = endTimeSetting;
            container->loadRawFile(eventsPath, &opt);
        } else if (eventsPath.size() >= 7 && eventsPath.compare(eventsPath.size() - 7, 7, ".aedat4") == 0) {
            // an iniVation DV recording (AEDAT 4: packets with LZ4 or no compression) inflated and decoded on the device.  Keys of this
            // build, all optional: Aedat4_Stream (the stream id of the events; absent: found by its identifier), Aedat4_TimeBase
            // (microseconds of epoch time; absent: the first event's whole second), Aedat4_FlipX / Aedat4_FlipY (0).  Events outside
            // Camera.width x Camera.height are dropped.
            ecal_aedat4_options opt;
            ecal_aedat4_default_options(&opt);
            if (!fsSettings["Aedat4_Stream"].isNone()) opt.stream_id = (int) fsSettings["Aedat4_Stream"];
            if (!fsSettings["Aedat4_TimeBase"].isNone()) {
                opt.auto_time_base = 0;
                opt.time_base = std::strtoll(((std::string) fsSettings["Aedat4_TimeBase"]).c_str(), nullptr, 10);
            }
            if (!fsSettings["Aedat4_FlipX"].isNone()) opt.flip_x = (int) fsSettings["Aedat4_FlipX"] ? 1 : 0;
            if (!fsSettings["Aedat4_FlipY"].isNone()) opt.flip_y = (int) fsSettings["Aedat4_FlipY"] ? 1 : 0;
            opt.width = (uint32_t) width;
            opt.height = (uint32_t) height;
            opt.start_time = startTime;
            opt.has_end_time = customEnd ? 1 : 0;
            opt.end_time = endTimeSetting;
            try {
                container->loadAedat4File(eventsPath, &opt);
            } catch (const std::exception &e) {   // (ZSTD packets, a stereo recording, a broken frame, a file cut short: said plainly)
                std::fprintf(stderr, "%s\n", e.what());
                return 4;
            }
            std::printf("aedat4_time_base %lld\n", (long long) container->aedat4Info.time_base);   // microseconds: t = 0 of this run
        } else if (eventsPath.size() >= 6 && eventsPath.compare(eventsPath.size() - 6, 6, ".aedat") == 0) {
            // an iniVation recording (AEDAT 3.1 / 2.0, the version from its first line) decoded on the device.  Keys of this build,
            // all optional: Aedat_TimeBase (microseconds of the camera's clock, 0), Aedat_FlipX / Aedat_FlipY (0; which a
            // recorder's files need is the user's knowledge), Aedat_Source (3.1: only polarity packets of this eventSource; absent:
            // every source).  Events outside Camera.width x Camera.height are dropped.
            ecal_aedat_options opt;
            ecal_aedat_default_options(&opt);
            if (!fsSettings["Aedat_TimeBase"].isNone()) opt.time_base = std::strtoll(((std::string) fsSettings["Aedat_TimeBase"]).c_str(), nullptr, 10);
            if (!fsSettings["Aedat_FlipX"].isNone()) opt.flip_x = (int) fsSettings["Aedat_FlipX"] ? 1 : 0;
            if (!fsSettings["Aedat_FlipY"].isNone()) opt.flip_y = (int) fsSettings["Aedat_FlipY"] ? 1 : 0;
            if (!fsSettings["Aedat_Source"].isNone()) opt.source = (int) fsSettings["Aedat_Source"];
            opt.width = (uint32_t) width;
            opt.height = (uint32_t) height;
            opt.start_time = startTime;
            opt.has_end_time = customEnd ? 1 : 0;
            opt.end_time = endTimeSetting;
            try {
                container->loadAedatFile(eventsPath, &opt);
            } catch (const std::exception &e) {   // (a version that is not read, a broken packet: said plainly, no abort)
                std::fprintf(stderr, "%s\n", e.what());
                return 4;
            }
        } else if (eventsPath.size() >= 4 && eventsPath.compare(eventsPath.size() - 4, 4, ".bag") == 0) {
            // a ROS 1 bag of dvs_msgs/EventArray messages (as rpg_dvs_ros records them) decoded on the device.  Keys of this build,
            // all optional: Bag_Topic (absent: the one topic of events), Bag_Type (absent: dvs_msgs/EventArray and
            // prophesee_event_msgs/EventArray), Bag_TimeBase (nanoseconds of epoch time; absent: the first event's whole second),
            // Bag_FlipX / Bag_FlipY (0).  Events outside Camera.width x Camera.height are dropped.
            ecal_bag_options opt;
            ecal_bag_default_options(&opt);
            std::string bagTopic, bagType;
            if (!fsSettings["Bag_Topic"].isNone()) bagTopic = (std::string) fsSettings["Bag_Topic"];
            if (!fsSettings["Bag_Type"].isNone()) bagType = (std::string) fsSettings["Bag_Type"];
            opt.topic = bagTopic.c_str();
            opt.type = bagType.c_str();
            if (!fsSettings["Bag_TimeBase"].isNone()) {
                opt.auto_time_base = 0;
                opt.time_base = std::strtoll(((std::string) fsSettings["Bag_TimeBase"]).c_str(), nullptr, 10);
            }
            if (!fsSettings["Bag_FlipX"].isNone()) opt.flip_x = (int) fsSettings["Bag_FlipX"] ? 1 : 0;
            if (!fsSettings["Bag_FlipY"].isNone()) opt.flip_y = (int) fsSettings["Bag_FlipY"] ? 1 : 0;
            opt.width = (uint32_t) width;
            opt.height = (uint32_t) height;
            opt.start_time = startTime;
            opt.has_end_time = customEnd ? 1 : 0;
            opt.end_time = endTimeSetting;
            try {
                container->loadBagFile(eventsPath, &opt);
            } catch (const std::exception &e) {   // (compressed chunks, a ROS 2 file, another message layout: said plainly, no abort)
                std::fprintf(stderr, "%s\n", e.what());
                return 4;
            }
            std::printf("bag_time_base %lld\n", (long long) container->bagInfo.time_base);   // nanoseconds: t = 0 of this run
        } else if (eventsPath.size() >= 5 && eventsPath.compare(eventsPath.size() - 5, 5, ".mcap") == 0) {
            // a ROS 2 MCAP recording of event messages (dvs_msgs / prophesee_event_msgs EventArray, event_camera_msgs EventPacket with
            // mono or evt3 packets) decoded on the device.  Keys of this build, all optional: Mcap_Topic (absent: the one topic of
            // events), Mcap_TimeBase (nanoseconds of epoch time, evt3: microseconds of the camera's clock; absent: the first event's
            // whole second, evt3: 0), Mcap_FlipX / Mcap_FlipY (0; not for evt3).  Events outside Camera.width x Camera.height are dropped.
            ecal_mcap_options opt;
            ecal_mcap_default_options(&opt);
            std::string mcapTopic;
            if (!fsSettings["Mcap_Topic"].isNone()) mcapTopic = (std::string) fsSettings["Mcap_Topic"];
            opt.topic = mcapTopic.c_str();
            if (!fsSettings["Mcap_TimeBase"].isNone()) {
                opt.auto_time_base = 0;
                opt.time_base = std::strtoll(((std::string) fsSettings["Mcap_TimeBase"]).c_str(), nullptr, 10);
            }
            if (!fsSettings["Mcap_FlipX"].isNone()) opt.flip_x = (int) fsSettings["Mcap_FlipX"] ? 1 : 0;
            if (!fsSettings["Mcap_FlipY"].isNone()) opt.flip_y = (int) fsSettings["Mcap_FlipY"] ? 1 : 0;
            opt.width = (uint32_t) width;
            opt.height = (uint32_t) height;
            opt.start_time = startTime;
            opt.has_end_time = customEnd ? 1 : 0;
            opt.end_time = endTimeSetting;
            try {
                container->loadMcapFile(eventsPath, &opt);
            } catch (const std::exception &e) {   // (compressed chunks, a stereo file, another message layout or codec: said plainly, no abort)
                std::fprintf(stderr, "%s\n", e.what());
                return 4;
            }
            std::printf("mcap_time_base %lld\n", (long long) container->mcapInfo.time_base);   // t = 0 of this run
        } else if (eventsPath.size() >= 4 && eventsPath.compare(eventsPath.size() - 4, 4, ".npy") == 0) {
            // events as numpy saves them — a 1-D structured array with fields t|ts|time|timestamp, x, y, p|pol|polarity, or an (N, 4)
            // array — decoded on the device.  Keys of this build, all optional: Npy_TimeMagnitude (seconds per tick, 1e-6; 1 for
            // stamps in seconds), Npy_TimeBase (ticks, 0), Npy_Columns (of an (N, 4) array, "txyp"), Npy_FlipX / Npy_FlipY (0).
            // Events outside Camera.width x Camera.height are dropped.
            ecal_npy_options opt;
            ecal_npy_default_options(&opt);
            std::string npyColumns;
            if (!fsSettings["Npy_TimeMagnitude"].isNone()) fsSettings["Npy_TimeMagnitude"] >> opt.fields.time_magnitude;
            if (!fsSettings["Npy_TimeBase"].isNone()) opt.fields.time_base = std::strtoll(((std::string) fsSettings["Npy_TimeBase"]).c_str(), nullptr, 10);
            if (!fsSettings["Npy_Columns"].isNone()) npyColumns = (std::string) fsSettings["Npy_Columns"];
            opt.columns = npyColumns.c_str();
            if (!fsSettings["Npy_FlipX"].isNone()) opt.fields.flip_x = (int) fsSettings["Npy_FlipX"] ? 1 : 0;
            if (!fsSettings["Npy_FlipY"].isNone()) opt.fields.flip_y = (int) fsSettings["Npy_FlipY"] ? 1 : 0;
            opt.fields.width = (uint32_t) width;
            opt.fields.height = (uint32_t) height;
            opt.fields.start_time = startTime;
            opt.fields.has_end_time = customEnd ? 1 : 0;
            opt.fields.end_time = endTimeSetting;
            try {
                container->loadNpyFile(eventsPath, &opt);
            } catch (const std::exception &e) {   // (a big-endian file, an object dtype, a missing field, a payload cut short: said plainly)
                std::fprintf(stderr, "%s\n", e.what());
                return 4;
            }
        } else {
            container->loadFile(argv[2], startTime, customEnd, endTimeSetting);
        }
        // HotPixels (a key of this build, optional): 1 = the events of hot pixels — pixels that fire whatever the scene does — are
        // taken out of the loaded stream on the device (ecal_stream_remove_hot_pixels on Camera.width x Camera.height) before
        // anything looks at it, one line on stdout, the masked pixels with their counts in saveDir/HotPixels.txt.  The rule's
        // numbers, all optional: HotPixels_Factor (8), HotPixels_QuantilePermille (990), HotPixels_MinCount (64).  Absent or 0:
        // nothing changes
        int wantHotPixels = 0;
        fsSettings["HotPixels"] >> wantHotPixels;
        if (wantHotPixels) {
            ecal_hot_pixel_options opt;
            ecal_hot_pixel_default_options(&opt);
            opt.width = (uint32_t) width;
            opt.height = (uint32_t) height;
            int quantilePermille = (int) opt.quantile_permille, minCount = (int) opt.min_count;
            fsSettings["HotPixels_Factor"] >> opt.factor;
            fsSettings["HotPixels_QuantilePermille"] >> quantilePermille;
            fsSettings["HotPixels_MinCount"] >> minCount;
            opt.quantile_permille = (uint32_t) quantilePermille;   // (a negative number: refused by the library)
            opt.min_count = (uint32_t) std::max(0, minCount);
            const size_t plane = width > 0 && height > 0 ? (size_t) width * (size_t) height : 0;
            std::vector<uint8_t> hotMask(plane);
            std::vector<uint32_t> hotCounts(2 * plane);
            ecal_hot_pixel_info hp;
            try {
                container->removeHotPixels(&opt, &hp, hotMask.data(), hotCounts.data());
            } catch (const std::exception &e) {
                std::fprintf(stderr, "%s\n", e.what());
                return 4;
            }
            std::printf("hot pixels: %u pixels, %llu of %llu events removed\n", hp.n_hot_pixels, (unsigned long long) hp.n_removed,
                        (unsigned long long) hp.n_events);
            std::FILE *f = std::fopen((std::string(argv[3]) + "/HotPixels.txt").c_str(), "w");
            if (!f) {
                std::fprintf(stderr, "cannot write %s/HotPixels.txt\n", argv[3]);
                return 3;
            }
            for (size_t p = 0; p < plane; p++)   // x y count_negative count_positive
                if (hotMask[p]) std::fprintf(f, "%zu %zu %u %u\n", p % (size_t) width, p / (size_t) width, hotCounts[p], hotCounts[plane + p]);
            std::fclose(f);
        }
        // NoiseFilter (a key of this build, optional): 1 = the events without a recent neighbour event — background activity — are
        // taken out of the loaded stream on the device (ecal_stream_remove_noise on Camera.width x Camera.height), behind the hot
        // pixels when both keys are set; one line on stdout, the options and the totals in saveDir/NoiseFilter.txt.  The rule's
        // numbers, all optional: NoiseFilter_Dt (0.005 s), NoiseFilter_Radius (1), NoiseFilter_MinSupport (1), NoiseFilter_Self (0).
        // Absent or 0: nothing changes
        int wantNoiseFilter = 0;
        fsSettings["NoiseFilter"] >> wantNoiseFilter;
        if (wantNoiseFilter) {
            ecal_noise_options opt;
            ecal_noise_default_options(&opt);
            opt.width = (uint32_t) width;
            opt.height = (uint32_t) height;
            int radius = (int) opt.radius, minSupport = (int) opt.min_support, self = (int) opt.include_self;
            fsSettings["NoiseFilter_Dt"] >> opt.dt;
            fsSettings["NoiseFilter_Radius"] >> radius;
            fsSettings["NoiseFilter_MinSupport"] >> minSupport;
            fsSettings["NoiseFilter_Self"] >> self;
            opt.radius = (uint32_t) radius;   // (a negative number: refused by the library)
            opt.min_support = (uint32_t) std::max(0, minSupport);
            opt.include_self = (uint32_t) self;
            ecal_filter_totals nt;
            try {
                container->removeNoise(&opt, &nt);
            } catch (const std::exception &e) {
                std::fprintf(stderr, "%s\n", e.what());
                return 4;
            }
            std::printf("noise filter: %llu of %llu events removed\n", (unsigned long long) nt.n_removed, (unsigned long long) nt.n_events);
            std::FILE *f = std::fopen((std::string(argv[3]) + "/NoiseFilter.txt").c_str(), "w");
            if (!f) {
                std::fprintf(stderr, "cannot write %s/NoiseFilter.txt\n", argv[3]);
                return 3;
            }
            std::fprintf(f, "width %u\nheight %u\nradius %u\nmin_support %u\ninclude_self %u\ndt %.17g\n", opt.width, opt.height, opt.radius,
                         opt.min_support, opt.include_self, opt.dt);
            std::fprintf(f, "n_events %llu\nn_off_grid %llu\nn_removed %llu\nn_kept %llu\n", (unsigned long long) nt.n_events,
                         (unsigned long long) nt.n_off_grid, (unsigned long long) nt.n_removed, (unsigned long long) nt.n_kept);
            std::fclose(f);
        }
    }
    while (!es.isEnd()) {                                    // :154-163
        if (customEnd && es.current().timeStamp() >= endTimeSetting) break;
        if (es.current().timeStamp() >= startTime) container->emplace(es.current());
        es.next();
    }
    es.close();
    stage("load_file");
    (void) container->device();                              // the one upload (the reference fills its multimap here)
    stage("upload");
    const double endTime = container->lastTime();            // :165
    const int frameEventNumThreshold = fsSettings["FrameEventNumThreshold"];   // :168
    auto pattern = cs->circlePatternParameters;
    CirclesEventFrame::Params fp(fsSettings);                // :171
    // the reference's piece count (:172-173): 5 * (std::thread::hardware_concurrency() - 2) — the keyframe set depends on it (the
    // pieces' boundaries), so the same binary on the same box gives what the reference would; PieceNum (a key of this build,
    // optional) pins it where a result must not depend on the host (the tests do)
    int pieceNum = 5 * std::max(1, (int) std::thread::hardware_concurrency() - 2);
    fsSettings["PieceNum"] >> pieceNum;
    // GateMode (a key of this build, optional): 1 = ECAL_GATE_SHARED_MAP, the reference's semantics with one worker thread (the
    // default: one keyframe map for all pieces, TrackingBase.cpp:16-46, EventCalibIni.cpp:26-36); 0 = ECAL_GATE_OWN_PIECE, the
    // faster schedule-free gate (every piece's first success ungated)
    int gateMode = ECAL_GATE_SHARED_MAP;
    fsSettings["GateMode"] >> gateMode;
    std::vector<KeyFrame> kfs = detect_keyframes_device(*container, pattern, fp, step, frameEventNumThreshold, pieceNum, startTime, endTime, gateMode);
    std::printf("keyframes %zu\n", kfs.size());
    stage("keyframe_search");
    EventCalibIni ini(cs, step);
    EventCalibIni::Result res;
    std::vector<EventCalibSpline::Frame> frames;
    const size_t n_circ = (size_t) (pattern->rows * pattern->cols);
    // the rectify hook runs after K and the distortion are known (res is filled before the PnP loop)
    auto rectify = [&](size_t f, const EventCalibIni::FramePose &p) {
        CirclesEventFrame cf(container, kfs[f].duration, pattern, fp);
        if (!cf.extractFeatures()) return false;
        CirclesEventFrame::Camera cam{res.K[0], res.K[1], res.K[2], res.K[3], {0, 0, 0, 0, 0}};
        for (size_t i = 0; i < 5 && i < res.distCoeffs.size(); i++) cam.distCoeffs[i] = res.distCoeffs[i];
        cam.fisheye = cs->useFisheye;   // (4 coefficients k1..k4 then)
        double R[9], t[3];
        for (int i = 0; i < 9; i++) R[i] = p.Rsw[i];
        for (int i = 0; i < 3; i++) t[i] = p.tsw[i];
        if (!cf.rectifyFeatures({}, R, t, cam)) return false;
        frames.push_back(EventCalibSpline::makeFrame(kfs[f].timeStamp, p, cf.features(), cf.featureLandmark(), n_circ));
        return true;
    };
    // ... or for all keyframes at once, on the device
    std::vector<double> rect_feat;
    std::vector<uint32_t> rect_valid;
    auto rectify_all = [&](const std::vector<EventCalibIni::FramePose> &poses, const std::vector<char> &pnp_ok, std::vector<char> &ok) {
        const uint32_t F = (uint32_t) kfs.size();
        std::vector<double> dur(2 * (size_t) F), pose(12 * (size_t) F), lm(3 * n_circ);
        for (uint32_t f = 0; f < F; f++) {
            dur[2 * f] = kfs[f].duration.first;
            dur[2 * f + 1] = kfs[f].duration.second;
            for (int i = 0; i < 9; i++) pose[12 * (size_t) f + i] = poses[f].Rsw[i];
            for (int i = 0; i < 3; i++) pose[12 * (size_t) f + 9 + i] = poses[f].tsw[i];
        }
        for (int i = 0; i < pattern->rows; i++)
            for (int j = 0; j < pattern->cols; j++) {
                double *o = &lm[3 * (size_t) (i * pattern->cols + j)];
                o[0] = (float) ((pattern->isAsymmetric ? (2 * j + i % 2) : j) * pattern->squareSize);
                o[1] = (float) (i * pattern->squareSize);
                o[2] = 0;
            }
        CirclesEventFrame probe(container, kfs[0].duration, pattern, fp);
        ecal_detect_params dp;
        dp.dbscan_eps = fp.dbscan_eps;
        dp.dbscan_min_samples = (uint32_t) fp.dbscan_startMinSample;
        dp.cluster_min_sample = (uint32_t) fp.clusterMinSample;
        dp.need_clusters = (uint32_t) n_circ;
        dp.circle_radius_threshold = probe.circleRadiusThreshold();
        dp.fit_circle = fp.fitCircle ? 1 : 0;
        dp.knn_num = (uint32_t) fp.knn_num;
        dp.rows = (uint32_t) pattern->rows;
        dp.cols = (uint32_t) pattern->cols;
        ecal_rectify_params rp;
        rp.fx = res.K[0], rp.fy = res.K[1], rp.cx = res.K[2], rp.cy = res.K[3];
        for (size_t i = 0; i < 5; i++) rp.dist[i] = i < res.distCoeffs.size() ? res.distCoeffs[i] : 0.0;
        rp.width = container->cameraSize[0], rp.height = container->cameraSize[1];
        rp.rows = (uint32_t) pattern->rows, rp.cols = (uint32_t) pattern->cols;
        rp.asymmetric = pattern->isAsymmetric ? 1 : 0;
        rp.circle_radius = pattern->circleRadius;
        rp.fit_circle = fp.fitCircle ? 1 : 0;
        rp.model = cs->useFisheye ? 1 : 0;
        rect_feat.resize(3 * n_circ * (size_t) F);
        rect_valid.resize(n_circ * (size_t) F);
        std::vector<uint32_t> info(2 * (size_t) F);
        const int rc = ecal_rectify_keyframes(ecal_host::thread_ctx(), container->device(), dur.data(), F, &dp, pose.data(), lm.data(), &rp,
                                              rect_feat.data(), rect_valid.data(), info.data());
        if (rc != ECAL_OK) throw std::runtime_error(std::string("ecal_rectify_keyframes: ") + ecal_last_error(ecal_host::thread_ctx()));
        for (uint32_t f = 0; f < F; f++) ok[f] = pnp_ok[f] && info[2 * f] != 0;
    };
    if (!ini.cvCalibration(kfs, container->cameraSize[0], container->cameraSize[1], res, batch ? EventCalibIni::RectifyFn() : rectify,
                           batch ? EventCalibIni::BatchRectifyFn(rectify_all) : EventCalibIni::BatchRectifyFn()))
        return 1;
    if (batch)   // the accepted keyframes' frames from the batch's arrays
        for (size_t f : res.acceptedFrames) {
            std::vector<CirclesEventFrame::CalibCircle> feats;
            std::vector<int> lmk;
            for (size_t k = 0; k < n_circ; k++)
                if (rect_valid[f * n_circ + k]) {
                    const double *p = &rect_feat[3 * (f * n_circ + k)];
                    feats.push_back(CirclesEventFrame::CalibCircle{Vector2d{{p[0], p[1]}}, p[2]});
                    lmk.push_back((int) k);
                }
            frames.push_back(EventCalibSpline::makeFrame(kfs[f].timeStamp, res.poses[f], feats, lmk, n_circ));
        }
    stage("init_calibration_pnp_rectify");
    std::printf("init K %.9g %.9g %.9g %.9g rms %.6g accepted %zu checkPose %d rectify %d\n", res.K[0], res.K[1], res.K[2], res.K[3],
                res.rms, res.acceptedFrames.size(), res.discardedByCheckPose, res.discardedByRectify);
    double dist5[5] = {0, 0, 0, 0, 0};
    for (size_t i = 0; i < 5 && i < res.distCoeffs.size(); i++) dist5[i] = res.distCoeffs[i];
    bool useSO3 = false;
    fsSettings["useSO3"] >> useSO3;                          // :204-206 (reduceMap: experimental in the reference, not restated)
    // CalibrationReport (a key of this build, optional): 1 = the residuals at the solution binned on the GPU (ecal_solver_report)
    // and written to saveDir/CalibrationReport.txt; absent or 0: nothing changes
    int wantReport = 0;
    fsSettings["CalibrationReport"] >> wantReport;
    ecal_report_options reportOptions;
    ecal_report_default_options(&reportOptions);
    reportOptions.width = (uint32_t) width;
    reportOptions.height = (uint32_t) height;
    // CalibrationReportPixels (a key of this build, optional): 1 = the same report in PIXELS (ecal_solver_report_px: per residual the
    // first-order distance from the event to the projected rim) written to saveDir/CalibrationReportPixels.txt, the layout of
    // CalibrationReport.txt; absent or 0: nothing changes
    int wantReportPx = 0;
    fsSettings["CalibrationReportPixels"] >> wantReportPx;
    ecal_report_options reportPxOptions;
    ecal_report_px_default_options(&reportPxOptions);
    reportPxOptions.width = (uint32_t) width;
    reportPxOptions.height = (uint32_t) height;
    // CalibrationUncertainty / CalibrationUncertainty_ClusterSpans (keys of this build, optional): 1 = the formal and the cluster-robust
    // covariance of the nine intrinsics at the solution (ecal_solver_uncertainty, include/ecal_uncertainty.h; clusters of
    // CalibrationUncertainty_ClusterSpans knot spans, absent or < 1: 1) written to saveDir/CalibrationUncertainty.txt, and the per-pixel
    // sigma of the bearing under the robust covariance (the formal one where the robust one is not valid) to
    // saveDir/uncertainty_sigma_px.npy (f32 (height, width), 0 where the model is invalid); absent or 0: nothing changes
    int wantUncertainty = 0, uncertaintyClusterSpans = 1;
    fsSettings["CalibrationUncertainty"] >> wantUncertainty;
    fsSettings["CalibrationUncertainty_ClusterSpans"] >> uncertaintyClusterSpans;
    if (uncertaintyClusterSpans < 1) uncertaintyClusterSpans = 1;
    // BoardImage (a key of this build, optional): 1 = every event of the stream carried through the solution onto the board
    // (ecal_solver_board_image), written to saveDir/board_image.png and saveDir/BoardImage.txt; absent or 0: nothing changes
    int wantBoardImage = 0;
    fsSettings["BoardImage"] >> wantBoardImage;
    // RefineRounds / RefineRingTol (keys of this build, optional): N rounds of re-association through the solution — every event of
    // the stream within RefineRingTol board units (absent or <= 0: the Huber width) of a circle's rim becomes a residual — each
    // followed by a solve from that solution, one `refine round k ...` line per round; absent or 0: nothing changes
    int refineRounds = 0;
    fsSettings["RefineRounds"] >> refineRounds;
    double refineRingTol = 0.0;
    fsSettings["RefineRingTol"] >> refineRingTol;
    // UndistortedEvents / UndistortedEvents_Pixel / UndistortedImages (keys of this build, optional): the solved camera applied to
    // the stream the calibration ran on (include/ecal.h, "undistortion").  UndistortedEvents: 1 writes saveDir/events_undistorted.bin,
    // the records with sub-pixel coordinates — with UndistortedEvents_Pixel: 1 the pixels of the reference's canvas (round(1.2 * size),
    // events outside it dropped).  UndistortedImages: 1 writes EventFrame::undistortedImage of every accepted keyframe to
    // saveDir/undistortedImage/<std::to_string(timeStamp)>_undistorted.png (the folder and names visulization_eventCalib.cpp:85-93
    // reads).  Either writes saveDir/Undistorted.txt.  Absent or 0: nothing changes
    int wantUndistortedEvents = 0, wantUndistortedPixel = 0, wantUndistortedImages = 0;
    fsSettings["UndistortedEvents"] >> wantUndistortedEvents;
    fsSettings["UndistortedEvents_Pixel"] >> wantUndistortedPixel;
    fsSettings["UndistortedImages"] >> wantUndistortedImages;
    const bool wantUndistort = wantUndistortedEvents || wantUndistortedImages;
    // UndistortMaps / UndistortMaps_Reference (keys of this build, optional): the solved camera's rectification maps (include/ecal.h,
    // "image undistortion": cv::initUndistortRectifyMap's CV_32FC1 convention, ready for cv::remap).  UndistortMaps: 1 writes
    // saveDir/undistort_map_x.npy and undistort_map_y.npy (f32 (out_height, out_width), numpy.load reads them) on the sensor's own canvas —
    // with UndistortMaps_Reference: 1 on the reference's (round(1.2 * size), offsets round(size * 0.1)) — and saveDir/UndistortMaps.txt.
    // Absent or 0: nothing changes
    int wantUndistortMaps = 0, wantUndistortMapsReference = 0;
    fsSettings["UndistortMaps"] >> wantUndistortMaps;
    fsSettings["UndistortMaps_Reference"] >> wantUndistortMapsReference;
    EventCalibSpline spline(frames, container, pattern, useSO3, step, res.K, dist5, 50, cs->useFisheye, wantReport ? &reportOptions : nullptr,
                            wantBoardImage != 0, refineRounds, refineRingTol, wantUndistort, wantReportPx ? &reportPxOptions : nullptr,
                            wantUncertainty ? uncertaintyClusterSpans : 0);
    const double *x = spline.intrinsics();
    std::printf("refined %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g residuals %zu iterations %d splines %zu\n", x[0], x[1], x[2], x[3],
                x[4], x[5], x[6], x[7], x[8], spline.summary().residuals, spline.summary().iterations, spline.splineNum());
    for (size_t k = 0; k < spline.refine().size(); k++) {
        const EventCalibSpline::RefineRound &r = spline.refine()[k];
        std::printf("refine round %zu events %llu kept %llu cost %.9g -> %.9g iterations %d\n", k, (unsigned long long) r.totals.n_events,
                    (unsigned long long) r.totals.n_kept, r.initial_cost, r.final_cost, r.iterations);
    }
    stage("spline_fit_association_lm");
    spline.saveKeyFrameTrajectoryTUM(std::string(argv[3]) + "/TrajectoryByEvent.txt");   // :212
    stage("save_trajectory");
    if (!batch) {   // :214-227: saveDir/image/<std::to_string(time stamp)>.png of every keyframe in the map
        const std::string dir = std::string(argv[3]) + "/image";
        std::error_code ec;
        std::filesystem::remove_all(dir, ec);
        std::filesystem::create_directories(dir, ec);
        size_t written = 0;
        for (size_t f : res.acceptedFrames) {
            CirclesEventFrame cf(container, kfs[f].duration, pattern, fp);
            (void) cf.extractFeatures();
            if (ecal_host::write_png_rgb(dir + "/" + std::to_string(kfs[f].timeStamp) + ".png", (int) container->cameraSize[0],
                                         (int) container->cameraSize[1], cf.image()))
                written++;
        }
        std::printf("images %zu\n", written);
    }
    if (wantUndistort) {
        ecal_ctx *ctx = ecal_host::thread_ctx();
        ecal_undistort_camera cam;
        ecal_undistort_camera_from_params(cs->useFisheye ? ECAL_CAMERA_FISHEYE : ECAL_CAMERA_RADIAL, x, &cam);
        ecal_undistort_options canvas;
        ecal_undistort_reference_canvas((uint32_t) width, (uint32_t) height, &canvas);
        std::FILE *f = std::fopen((std::string(argv[3]) + "/Undistorted.txt").c_str(), "w");
        if (!f) {
            std::fprintf(stderr, "cannot write %s/Undistorted.txt\n", argv[3]);
            return 3;
        }
        std::fprintf(f, "model %d\nintrinsics %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\nout_k %.17g %.17g %.17g %.17g\n", cam.model,
                     x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8], cam.out_k[0], cam.out_k[1], cam.out_k[2], cam.out_k[3]);
        try {
            if (wantUndistortedEvents) {
                ecal_undistort_options opt = canvas;
                if (!wantUndistortedPixel) std::memset(&opt, 0, sizeof(opt));   // ECAL_UNDISTORT_SUBPIXEL
                ecal_undistort_totals t;
                EventContainer::Ptr und = container->undistorted(cam, &opt, &t);
                const std::string bin = std::string(argv[3]) + "/events_undistorted.bin";
                if (ecal_stream_to_bin_file(ctx, und->device(), bin.c_str()) != ECAL_OK) {
                    std::fprintf(stderr, "%s\n", ecal_last_error(ctx));
                    std::fclose(f);
                    return 3;
                }
                std::fprintf(f, "events mode %u out_width %u out_height %u off_x %.17g off_y %.17g\n", opt.mode, opt.out_width, opt.out_height,
                             opt.off_x, opt.off_y);
                std::fprintf(f, "events n_events %llu n_invalid %llu n_outside %llu n_kept %llu\n", (unsigned long long) t.n_events,
                             (unsigned long long) t.n_invalid, (unsigned long long) t.n_outside, (unsigned long long) t.n_kept);
                std::printf("undistorted events %llu of %llu kept\n", (unsigned long long) t.n_kept, (unsigned long long) t.n_events);
            }
            if (wantUndistortedImages) {
                const std::string dir = std::string(argv[3]) + "/undistortedImage";
                std::error_code ec;
                std::filesystem::remove_all(dir, ec);
                std::filesystem::create_directories(dir, ec);
                const std::vector<size_t> &acc = res.acceptedFrames;
                const size_t pic = (size_t) canvas.out_width * canvas.out_height * 3, batchFrames = 64;
                std::vector<uint8_t> rgb, one(pic);
                unsigned long long sums[4] = {0, 0, 0, 0};
                size_t written = 0;
                for (size_t at = 0; at < acc.size(); at += batchFrames) {
                    const size_t S = std::min(batchFrames, acc.size() - at);
                    std::vector<double> t0(S), t1(S);
                    std::vector<ecal_undistort_frame_totals> ft(S);
                    for (size_t k = 0; k < S; k++) {
                        t0[k] = kfs[acc[at + k]].duration.first;
                        t1[k] = kfs[acc[at + k]].duration.second;
                    }
                    rgb.resize(S * pic);
                    const int rc = ecal_stream_undistorted_frames(ctx, container->device(), &cam, &canvas, t0.data(), t1.data(), (uint32_t) S, rgb.data(),
                                                                  ft.data());
                    if (rc != ECAL_OK) throw std::runtime_error(std::string("ecal_stream_undistorted_frames: ") + ecal_last_error(ctx));
                    for (size_t k = 0; k < S; k++) {
                        one.assign(rgb.begin() + k * pic, rgb.begin() + (k + 1) * pic);
                        if (ecal_host::write_png_rgb(dir + "/" + std::to_string(kfs[acc[at + k]].timeStamp) + "_undistorted.png", (int) canvas.out_width,
                                                     (int) canvas.out_height, one))
                            written++;
                        sums[0] += ft[k].n_pos, sums[1] += ft[k].n_neg, sums[2] += ft[k].n_invalid, sums[3] += ft[k].n_outside;
                    }
                }
                std::fprintf(f, "images %zu out_width %u out_height %u off_x %.17g off_y %.17g\n", written, canvas.out_width, canvas.out_height,
                             canvas.off_x, canvas.off_y);
                std::fprintf(f, "images n_pos %llu n_neg %llu n_invalid %llu n_outside %llu\n", sums[0], sums[1], sums[2], sums[3]);
                std::printf("undistorted images %zu\n", written);
            }
        } catch (const std::exception &e) {
            std::fprintf(stderr, "%s\n", e.what());
            std::fclose(f);
            return 4;
        }
        std::fclose(f);
        container->release();
    }
    if (wantUndistortMaps) {
        std::vector<float> mapX, mapY;
        ecal_image_info info;
        try {
            PinholeCamera solved({(double) width, (double) height}, {x[0], 0.0, x[2], 0.0, x[1], x[3], 0.0, 0.0, 1.0},
                                 std::vector<double>(x + 4, x + 9), cs->useFisheye);
            info = solved.undistortMaps(mapX, mapY, wantUndistortMapsReference != 0);
        } catch (const std::exception &e) {
            std::fprintf(stderr, "%s\n", e.what());
            return 4;
        }
        const ecal_image_options &o = info.opt;
        const std::string dir = argv[3];
        std::FILE *f = std::fopen((dir + "/UndistortMaps.txt").c_str(), "w");
        if (!f || !ecal_host::write_npy_f32(dir + "/undistort_map_x.npy", o.out_height, o.out_width, mapX.data()) ||
            !ecal_host::write_npy_f32(dir + "/undistort_map_y.npy", o.out_height, o.out_width, mapY.data())) {
            std::fprintf(stderr, "cannot write the undistortion maps under %s\n", argv[3]);
            if (f) std::fclose(f);
            return 3;
        }
        std::fprintf(f, "model %d\nintrinsics %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\nout_k %.17g %.17g %.17g %.17g\n",
                     cs->useFisheye ? ECAL_CAMERA_FISHEYE : ECAL_CAMERA_RADIAL, x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8], x[0], x[1], x[2],
                     x[3]);
        std::fprintf(f, "options method %u channels %u out_width %u out_height %u normalize %u off_x %.17g off_y %.17g\n", o.method, o.channels,
                     o.out_width, o.out_height, o.normalize, o.off_x, o.off_y);
        std::fprintf(f, "info width %u height %u r_lim %.17g truncated %u n_invalid %llu n_not_converged %llu n_empty %llu bytes %llu\n", info.width,
                     info.height, info.r_lim, info.truncated, (unsigned long long) info.n_invalid, (unsigned long long) info.n_not_converged,
                     (unsigned long long) info.n_empty, (unsigned long long) info.bytes);
        std::fclose(f);
        std::printf("undistort maps %u x %u invalid %llu\n", o.out_width, o.out_height, (unsigned long long) info.n_invalid);
    }
    if (wantReport && spline.report().valid) {
        const EventCalibSpline::Report &rp = spline.report();
        using Rp = EventCalibSpline::Report;
        const ecal_bin_stats &a = rp.totals.all;
        std::FILE *f = std::fopen((std::string(argv[3]) + "/CalibrationReport.txt").c_str(), "w");
        if (!f) {
            std::fprintf(stderr, "cannot write %s/CalibrationReport.txt\n", argv[3]);
            return 3;
        }
        auto line = [&](const char *tag, size_t id, const ecal_bin_stats &b) {
            std::fprintf(f, "%s %zu n %llu n_out %llu rms %.9g mean %.9g mean_abs %.9g max_abs %.9g\n", tag, id, (unsigned long long) b.n,
                         (unsigned long long) b.n_out, Rp::rms(b), b.n ? b.sum_r / (double) b.n : 0.0, b.n ? b.sum_abs / (double) b.n : 0.0,
                         b.max_abs);
        };
        std::fprintf(f, "# residuals in board units (the unit of Circles_Radius); outlier: |r| > %.9g\n",
                     rp.options.outlier_thresh > 0 ? rp.options.outlier_thresh : 0.2 * pattern->circleRadius);
        std::fprintf(f, "totals n %llu n_out %llu sum_r %.17g sum_r2 %.17g sum_abs %.17g max_abs %.17g cost %.17g rms %.9g\n",
                     (unsigned long long) a.n, (unsigned long long) a.n_out, a.sum_r, a.sum_r2, a.sum_abs, a.max_abs, rp.totals.cost, Rp::rms(a));
        std::vector<size_t> order;
        for (size_t k = 0; k < rp.keyframes.size(); k++)
            if (rp.keyframes[k].n) order.push_back(k);
        std::stable_sort(order.begin(), order.end(), [&](size_t i, size_t j) { return Rp::rms(rp.keyframes[i]) > Rp::rms(rp.keyframes[j]); });
        std::fprintf(f, "worst_keyframes %zu of %zu\n", std::min<size_t>(10, order.size()), rp.keyframes.size());
        for (size_t k = 0; k < order.size() && k < 10; k++) {
            std::fprintf(f, "t %.6f ", spline.frames()[order[k]].timeStamp);
            line("keyframe", order[k], rp.keyframes[order[k]]);
        }
        std::fprintf(f, "landmarks %zu\n", rp.landmarks.size());
        for (size_t k = 0; k < rp.landmarks.size(); k++) line("landmark", k, rp.landmarks[k]);
        std::fprintf(f, "coverage %u %u cell_px %u\n", rp.cells_y, rp.cells_x, rp.options.cell_px);
        for (uint32_t y = 0; y < rp.cells_y; y++) {
            for (uint32_t x2 = 0; x2 < rp.cells_x; x2++)
                std::fprintf(f, x2 ? " %llu" : "%llu", (unsigned long long) rp.cell_n[(size_t) y * rp.cells_x + x2]);
            std::fprintf(f, "\n");
        }
        std::fprintf(f, "empty_cells %.6f\n", rp.emptyCellFraction());
        std::fprintf(f, "histogram %zu range %.9g\n", rp.hist.size(), rp.hist_range);
        for (size_t k = 0; k < rp.hist.size(); k++) std::fprintf(f, k ? " %llu" : "%llu", (unsigned long long) rp.hist[k]);
        std::fprintf(f, "\n");
        std::fclose(f);
        std::printf("report rms %.9g outliers %.6f empty_cells %.6f\n", Rp::rms(a), rp.outlierFraction(), rp.emptyCellFraction());
    }
    if (wantReportPx && spline.reportPx().valid) {
        const EventCalibSpline::ReportPx &rp = spline.reportPx();
        using Rp = EventCalibSpline::Report;
        const ecal_bin_stats &a = rp.totals.all;
        std::FILE *f = std::fopen((std::string(argv[3]) + "/CalibrationReportPixels.txt").c_str(), "w");
        if (!f) {
            std::fprintf(stderr, "cannot write %s/CalibrationReportPixels.txt\n", argv[3]);
            return 3;
        }
        auto line = [&](const char *tag, size_t id, const ecal_bin_stats &b) {
            std::fprintf(f, "%s %zu n %llu n_out %llu rms %.9g mean %.9g mean_abs %.9g max_abs %.9g\n", tag, id, (unsigned long long) b.n,
                         (unsigned long long) b.n_out, Rp::rms(b), b.n ? b.sum_r / (double) b.n : 0.0, b.n ? b.sum_abs / (double) b.n : 0.0,
                         b.max_abs);
        };
        std::fprintf(f, "# residuals in pixels (first-order distance to the projected rim); px_per_unit %.9g; outlier: |r| > %.9g\n",
                     rp.pxPerUnit(), rp.outlier_thresh);
        std::fprintf(f, "totals n %llu n_out %llu sum_r %.17g sum_r2 %.17g sum_abs %.17g max_abs %.17g n_degenerate %llu sum_px_per_unit %.17g rms %.9g\n",
                     (unsigned long long) a.n, (unsigned long long) a.n_out, a.sum_r, a.sum_r2, a.sum_abs, a.max_abs,
                     (unsigned long long) rp.totals.n_degenerate, rp.totals.sum_px_per_unit, rp.rmsPx());
        std::vector<size_t> order;
        for (size_t k = 0; k < rp.keyframes.size(); k++)
            if (rp.keyframes[k].n) order.push_back(k);
        std::stable_sort(order.begin(), order.end(), [&](size_t i, size_t j) { return Rp::rms(rp.keyframes[i]) > Rp::rms(rp.keyframes[j]); });
        std::fprintf(f, "worst_keyframes %zu of %zu\n", std::min<size_t>(10, order.size()), rp.keyframes.size());
        for (size_t k = 0; k < order.size() && k < 10; k++) {
            std::fprintf(f, "t %.6f ", spline.frames()[order[k]].timeStamp);
            line("keyframe", order[k], rp.keyframes[order[k]]);
        }
        std::fprintf(f, "landmarks %zu\n", rp.landmarks.size());
        for (size_t k = 0; k < rp.landmarks.size(); k++) line("landmark", k, rp.landmarks[k]);
        std::fprintf(f, "coverage %u %u cell_px %u\n", rp.cells_y, rp.cells_x, rp.options.cell_px);
        for (uint32_t y = 0; y < rp.cells_y; y++) {
            for (uint32_t x2 = 0; x2 < rp.cells_x; x2++)
                std::fprintf(f, x2 ? " %llu" : "%llu", (unsigned long long) rp.cell_n[(size_t) y * rp.cells_x + x2]);
            std::fprintf(f, "\n");
        }
        std::fprintf(f, "empty_cells %.6f\n", rp.emptyCellFraction());
        std::fprintf(f, "histogram %zu range %.9g\n", rp.hist.size(), rp.hist_range);
        for (size_t k = 0; k < rp.hist.size(); k++) std::fprintf(f, k ? " %llu" : "%llu", (unsigned long long) rp.hist[k]);
        std::fprintf(f, "\n");
        std::fclose(f);
        std::printf("report_px rms_px %.9g px_per_unit %.9g outliers %.6f degenerate %llu\n", rp.rmsPx(), rp.pxPerUnit(), rp.outlierFraction(),
                    (unsigned long long) rp.totals.n_degenerate);
    }
    if (wantUncertainty && spline.uncertainty().valid) {
        const ecal_uncertainty_result &u = spline.uncertainty().result;
        static const char *const names[9] = {"fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4", "k5"};
        std::FILE *f = std::fopen((std::string(argv[3]) + "/CalibrationUncertainty.txt").c_str(), "w");
        if (!f) {
            std::fprintf(stderr, "cannot write %s/CalibrationUncertainty.txt\n", argv[3]);
            return 3;
        }
        std::fprintf(f, "# sigma: formal, s2 (H^-1)_intr, assumes independent residuals; sigma_robust: clusters of %u knot span(s); inflation = sigma_robust / sigma\n",
                     spline.uncertainty().clusterSpans);
        std::fprintf(f, "counts n_res %llu n_unknowns %u n_cp %u n_chunks %u n_clusters %u cluster_spans %u\n", (unsigned long long) u.n_res, u.n_unknowns,
                     u.n_cp, u.n_chunks, u.n_clusters, spline.uncertainty().clusterSpans);
        std::fprintf(f, "flags positive_definite %u formal_valid %u robust_valid %u\n", u.positive_definite, u.formal_valid, u.robust_valid);
        std::fprintf(f, "cost %.17g s2 %.17g\n", u.cost, u.s2);
        for (int i = 0; i < 9; i++)
            std::fprintf(f, "intrinsic %s value %.17g sigma %.17g sigma_robust %.17g inflation %.9g\n", names[i], x[i], u.sigma[i], u.sigma_robust[i],
                         u.inflation[i]);
        std::fprintf(f, "correlation 9\n");
        for (int i = 0; i < 9; i++) {
            for (int j = 0; j < 9; j++) std::fprintf(f, j ? " %.17g" : "%.17g", u.corr[9 * i + j]);
            std::fprintf(f, "\n");
        }
        if (!u.positive_definite)
            std::fprintf(f, "# the normal matrix is not positive definite (a control point without residuals?): nothing below is a number\n");
        else if (!u.formal_valid || !u.robust_valid)
            std::fprintf(f, "# nan below: %s%s\n", u.formal_valid ? "" : "no formal figures (n_res <= n_unknowns) ",
                         u.robust_valid ? "" : "no robust figures (fewer than two clusters)");
        std::fprintf(f, "correlation_robust 9\n");   // cov_robust[i][j] / (sigma_robust[i] sigma_robust[j])
        for (int i = 0; i < 9; i++) {
            for (int j = 0; j < 9; j++) std::fprintf(f, j ? " %.17g" : "%.17g", u.cov_robust[9 * i + j] / (u.sigma_robust[i] * u.sigma_robust[j]));
            std::fprintf(f, "\n");
        }
        std::fclose(f);
        const bool robust = u.robust_valid != 0;
        double worst = 0.0;
        if (u.positive_definite && (robust || u.formal_valid)) {
            std::vector<double> sig((size_t) width * (size_t) height);
            std::vector<uint8_t> flag(sig.size());
            const int rc = ecal_uncertainty_map_host(cs->useFisheye ? ECAL_CAMERA_FISHEYE : ECAL_CAMERA_RADIAL, x, robust ? u.cov_robust : u.cov,
                                                     (uint32_t) width, (uint32_t) height, sig.data(), flag.data(), nullptr);
            if (rc != ECAL_OK) {
                std::fprintf(stderr, "ecal_uncertainty_map_host: %s\n", ecal_strerror(rc));
                return 3;
            }
            std::vector<float> sig32(sig.begin(), sig.end());
            for (double v : sig) worst = std::max(worst, v);
            if (!ecal_host::write_npy_f32(std::string(argv[3]) + "/uncertainty_sigma_px.npy", (size_t) height, (size_t) width, sig32.data())) {
                std::fprintf(stderr, "cannot write %s/uncertainty_sigma_px.npy\n", argv[3]);
                return 3;
            }
        }
        double maxInflation = std::nan("");   // (NaN unless both covariances hold numbers)
        if (u.formal_valid && u.robust_valid) maxInflation = *std::max_element(u.inflation, u.inflation + 9);
        std::printf("uncertainty clusters %u sigma_fx %.9g sigma_robust_fx %.9g max_inflation %.9g max_sigma_px %.9g\n", u.n_clusters, u.sigma[0],
                    u.sigma_robust[0], maxInflation, worst);
    }
    if (wantBoardImage && spline.boardImage().valid) {
        const EventCalibSpline::BoardImage &bi = spline.boardImage();
        using Bi = EventCalibSpline::BoardImage;
        const ecal_board_image_options &o = bi.options;
        const size_t plane = (size_t) o.width * o.height;
        // positive events in red and negative in green (the colours of EventFrame::undistortedImage, EventFrame.cpp:38-60), each
        // channel min(255, round(255 * count / p99)), p99 = the 99th percentile (nearest rank) of the non-zero counts of both planes
        std::vector<uint32_t> nz;
        for (uint32_t c : bi.image)
            if (c) nz.push_back(c);
        std::sort(nz.begin(), nz.end());
        const double p99 = nz.empty() ? 1.0 : (double) nz[(size_t) std::ceil(0.99 * (double) nz.size()) - 1];
        std::vector<uint8_t> rgb(3 * plane, 0);
        for (size_t i = 0; i < plane; i++) {
            rgb[3 * i] = (uint8_t) std::min(255.0, std::round(255.0 * bi.image[plane + i] / p99));
            rgb[3 * i + 1] = (uint8_t) std::min(255.0, std::round(255.0 * bi.image[i] / p99));
        }
        if (!ecal_host::write_png_rgb(std::string(argv[3]) + "/board_image.png", (int) o.width, (int) o.height, rgb)) {
            std::fprintf(stderr, "cannot write %s/board_image.png\n", argv[3]);
            return 3;
        }
        std::FILE *f = std::fopen((std::string(argv[3]) + "/BoardImage.txt").c_str(), "w");
        if (!f) {
            std::fprintf(stderr, "cannot write %s/BoardImage.txt\n", argv[3]);
            return 3;
        }
        const ecal_board_image_totals &t = bi.totals;
        std::fprintf(f, "# board units (the unit of Circles_Radius); d = distance to the nearest circle's centre - radius, |d| < %.9g\n", o.ring_range);
        std::fprintf(f, "totals n_events %llu n_outside_time %llu n_behind %llu n_outside_image %llu n_image_neg %llu n_image_pos %llu n_ring %llu\n",
                     (unsigned long long) t.n_events, (unsigned long long) t.n_outside_time, (unsigned long long) t.n_behind,
                     (unsigned long long) t.n_outside_image, (unsigned long long) t.n_image[0], (unsigned long long) t.n_image[1],
                     (unsigned long long) t.n_ring);
        std::fprintf(f, "image width %u height %u x0 %.17g y0 %.17g bin %.17g p99 %.9g\n", o.width, o.height, o.x0, o.y0, o.bin, p99);
        const size_t n_circ = bi.ring_stats.size() / 2;
        std::fprintf(f, "circles %zu\n", n_circ);
        ecal_ring_stats all{};
        for (size_t k = 0; k < n_circ; k++) {
            const ecal_ring_stats &ng = bi.ring_stats[2 * k], &ps = bi.ring_stats[2 * k + 1];
            std::fprintf(f, "circle %zu neg_n %llu neg_ring_mean %.9g neg_ring_std %.9g pos_n %llu pos_ring_mean %.9g pos_ring_std %.9g\n", k,
                         (unsigned long long) ng.n, Bi::mean(ng), Bi::stddev(ng), (unsigned long long) ps.n, Bi::mean(ps), Bi::stddev(ps));
            for (const ecal_ring_stats *r : {&ng, &ps}) {
                all.n += r->n;
                all.sum_d += r->sum_d;
                all.sum_d2 += r->sum_d2;
            }
        }
        std::fclose(f);
        std::printf("board_image events %llu in_image %llu ring %llu ring_mean %.9g ring_std %.9g\n", (unsigned long long) t.n_events,
                    (unsigned long long) (t.n_image[0] + t.n_image[1]), (unsigned long long) t.n_ring, Bi::mean(all), Bi::stddev(all));
    }
    return 0;
}
