// LabeledImage.hpp of the reference's DetectorTrainingApp (:20-86): an image with rectangular landmarks.  The landmark sources of
// imageio (dlib XML, ...) are not part of this backend; a LabeledImage is built from RectLandmarks directly.
#pragma once
#include <utility>
#include <vector>
#include "imageio/RectLandmark.hpp"

class LabeledImage {
public:
    LabeledImage(const cv::Mat& image, std::vector<imageio::RectLandmark> landmarks) : image(image), landmarks(std::move(landmarks)) {}
    // either the width or the height grows until the aspect ratio (width / height) is met
    void adjustSizes(double aspectRatio) {
        const double aspectRatioInv = 1.0 / aspectRatio;
        std::vector<imageio::RectLandmark> adjusted;
        for (const imageio::RectLandmark& landmark : landmarks) {
            float width = landmark.getWidth(), height = landmark.getHeight();
            if (width < aspectRatio * height) width = aspectRatio * height;
            else if (width > aspectRatio * height) height = width * aspectRatioInv;
            adjusted.emplace_back(landmark.getName(), landmark.getX(), landmark.getY(), width, height);
        }
        std::swap(landmarks, adjusted);
    }
    cv::Mat image;
    std::vector<imageio::RectLandmark> landmarks;
};
