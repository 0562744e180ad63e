// opengv2::PinholeCamera (core/sensor/include/opengv2/sensor/PinholeCamera.hpp) over the C ABI: the camera the solver found, with
// the members the reference's calibration app uses — undistortPoint, inverseRadialDistortion, undistortImage — and the two this
// project adds behind them, distortPoint and undistortMaps (include/ecal.h, "image undistortion").  Plain std types stand where the
// reference has Eigen and cv::Mat: a point is std::array<double, 2>, K is row major, a picture is interleaved u8 bytes.
#ifndef ECAL_HOST_PINHOLE_CAMERA_H_
#define ECAL_HOST_PINHOLE_CAMERA_H_

#include <array>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/ecal.h"
#include "dbscan.h"

namespace opengv2 {

class PinholeCamera {
public:
    // size: width, height; K: row major; inverseRadialPoly: k1..k5 of the solver (empty: no distortion); fisheye: the solver's
    // Kannala-Brandt form (a model of this project: the reference's class has the radial one alone)
    PinholeCamera(const std::array<double, 2> &size, const std::array<double, 9> &K, const std::vector<double> &inverseRadialPoly = {},
                  bool fisheye = false)
        : size_(size), K_(K), inverseRadialPoly_(inverseRadialPoly), fisheye_(fisheye) {}
    PinholeCamera(const PinholeCamera &) = delete;
    PinholeCamera &operator=(const PinholeCamera &) = delete;
    ~PinholeCamera() { ecal_image_plan_destroy(plan_); }

    const std::array<double, 2> &size() const noexcept { return size_; }
    const std::array<double, 9> &K() const noexcept { return K_; }
    void setK(const std::array<double, 9> &cameraMatrix) { K_ = cameraMatrix; }
    std::vector<double> &inverseRadialPoly() noexcept { return inverseRadialPoly_; }

    // PinholeCamera.cpp:69-95
    static std::vector<double> inverseRadialDistortion(const std::array<double, 4> &radialDistortion) {
        std::vector<double> b(5);
        ecal_inverse_radial_distortion(radialDistortion.data(), b.data());
        return b;
    }

    // the solver's parameter head fx fy cx cy k1..k5 with out_k = K, as the reference's K_ * Xc
    ecal_undistort_camera camera() const {
        double p[9] = {K_[0], K_[4], K_[2], K_[5], 0.0, 0.0, 0.0, 0.0, 0.0};
        if (inverseRadialPoly_.size() > 5) throw std::invalid_argument("PinholeCamera: at most five inverse radial coefficients");
        for (size_t i = 0; i < inverseRadialPoly_.size(); i++) p[4 + i] = inverseRadialPoly_[i];
        ecal_undistort_camera cam;
        ecal_undistort_camera_from_params(fisheye_ ? ECAL_CAMERA_FISHEYE : ECAL_CAMERA_RADIAL, p, &cam);
        return cam;
    }

    // PinholeCamera.cpp:97-126.  Without coefficients the point is handed back; an invalid point (ecal.h, "undistortion") throws
    std::array<double, 2> undistortPoint(const std::array<double, 2> &p) const {
        if (inverseRadialPoly_.empty()) return p;
        const ecal_undistort_camera cam = camera();
        std::array<double, 2> out{0.0, 0.0};
        uint8_t flag = 0;
        if (ecal_undistort_points_host(&cam, p.data(), 1, out.data(), &flag) != ECAL_OK)
            throw std::invalid_argument(std::string("undistortPoint: ") + (ecal_undistort_camera_error(&cam) ? ecal_undistort_camera_error(&cam) : "?"));
        if (flag) throw std::domain_error("undistortPoint: the point has no ideal position");
        return out;
    }

    // the forward projection, ideal pixel -> sensor pixel (not in the reference: its solved model has no closed form this way);
    // *valid (may be null: an invalid point throws) false beyond the radius up to which the model inverts
    std::array<double, 2> distortPoint(const std::array<double, 2> &p, bool *valid = nullptr) const {
        if (inverseRadialPoly_.empty()) {
            if (valid) *valid = true;
            return p;
        }
        const ecal_undistort_camera cam = camera();
        std::array<double, 2> out{0.0, 0.0};
        uint8_t flag = 0;
        if (ecal_distort_points_host(&cam, (uint32_t) size_[0], (uint32_t) size_[1], p.data(), 1, out.data(), &flag) != ECAL_OK)
            throw std::invalid_argument("distortPoint: the camera or its size is refused");
        if (valid) *valid = flag != ECAL_DISTORT_INVALID;
        else if (flag == ECAL_DISTORT_INVALID) throw std::domain_error("distortPoint: the point has no sensor position");
        return out;
    }

    // PinholeCamera.cpp:128-196: the picture on the canvas round(1.2 * size), min-max normalised.  image: height rows of
    // width * channels bytes; anything but 3 channels is refused as the reference refuses it.  The plan is built on the first call
    // and kept, as the reference keeps undistortMap_ (here it is built again when K or the coefficients have changed since).
    std::vector<uint8_t> undistortImage(const std::vector<uint8_t> &image, int channels = 3, int *widthOut = nullptr, int *heightOut = nullptr) {
        if (channels != 3) throw std::logic_error("only support CV_8UC3 for now.");
        const uint32_t W = (uint32_t) size_[0], H = (uint32_t) size_[1];
        if (image.size() != (size_t) W * H * 3) throw std::invalid_argument("undistortImage: the image is not width x height x 3 bytes");
        ecal_image_options opt;
        ecal_image_reference_options(W, H, &opt);
        if (inverseRadialPoly_.empty()) {   // (:211-213: the picture as it is)
            if (widthOut) *widthOut = (int) W;
            if (heightOut) *heightOut = (int) H;
            return image;
        }
        ecal_ctx *ctx = ecal_host::thread_ctx();
        const ecal_undistort_camera cam = camera();
        if (!plan_ || std::memcmp(&cam, &planCamera_, sizeof(cam)) != 0) {
            ecal_image_plan_destroy(plan_);
            plan_ = nullptr;
            const int rc = ecal_image_plan_create(ctx, &cam, W, H, &opt, &plan_);
            if (rc == ECAL_ERR_INVALID) throw std::invalid_argument(std::string("undistortImage: ") + ecal_last_error(ctx));
            if (rc != ECAL_OK) throw std::runtime_error(std::string("ecal_image_plan_create: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
            planCamera_ = cam;
            plansBuilt_++;
        }
        std::vector<uint8_t> dst((size_t) opt.out_width * opt.out_height * 3);
        const int rc = ecal_undistort_images(ctx, plan_, image.data(), 1, dst.data(), nullptr);
        if (rc != ECAL_OK) throw std::runtime_error(std::string("ecal_undistort_images: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        if (widthOut) *widthOut = (int) opt.out_width;
        if (heightOut) *heightOut = (int) opt.out_height;
        return dst;
    }

    // cv::initUndistortRectifyMap's CV_32FC1 maps for the new camera K on the sensor's own canvas (referenceCanvas: the canvas and
    // offsets of undistortImage): mapX, mapY [height][width], -1 where the forward projection has no sensor position
    ecal_image_info undistortMaps(std::vector<float> &mapX, std::vector<float> &mapY, bool referenceCanvas = false) const {
        const uint32_t W = (uint32_t) size_[0], H = (uint32_t) size_[1];
        ecal_image_options opt;
        ecal_image_reference_options(W, H, &opt);
        if (!referenceCanvas) opt.out_width = W, opt.out_height = H, opt.off_x = 0.0, opt.off_y = 0.0;
        opt.method = ECAL_IMAGE_BILINEAR, opt.channels = 1, opt.normalize = 0;
        ecal_ctx *ctx = ecal_host::thread_ctx();
        const ecal_undistort_camera cam = camera();
        ecal_image_plan *plan = nullptr;
        int rc = ecal_image_plan_create(ctx, &cam, W, H, &opt, &plan);
        if (rc == ECAL_ERR_INVALID) throw std::invalid_argument(std::string("undistortMaps: ") + ecal_last_error(ctx));
        if (rc != ECAL_OK) throw std::runtime_error(std::string("ecal_image_plan_create: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        ecal_image_info info;
        (void) ecal_image_plan_info(plan, &info);
        mapX.assign((size_t) opt.out_width * opt.out_height, 0.0f);
        mapY.assign(mapX.size(), 0.0f);
        rc = ecal_image_plan_maps(plan, mapX.data(), mapY.data(), nullptr);
        ecal_image_plan_destroy(plan);
        if (rc != ECAL_OK) throw std::runtime_error(std::string("ecal_image_plan_maps: ") + ecal_strerror(rc) + " — " + ecal_last_error(ctx));
        return info;
    }

    int plansBuilt() const noexcept { return plansBuilt_; }   // how often undistortImage built its plan

protected:
    std::array<double, 2> size_;
    std::array<double, 9> K_;
    // Inverse radial distortion polynomial (the solver's k1..k5)
    std::vector<double> inverseRadialPoly_;
    bool fisheye_ = false;
    // what the reference keeps in undistortMap_: the plan of the last camera undistortImage saw
    ecal_image_plan *plan_ = nullptr;
    ecal_undistort_camera planCamera_{};
    int plansBuilt_ = 0;
};

}  // namespace opengv2
#endif
