// Annotations.hpp of the reference's DetectorTrainingApp (:20-100): annotated bounding boxes, positive or fuzzy, never negative.
// A landmark is fuzzy when its name starts with "ignore" or both sides of its bounds are below minSize.
#pragma once
#include <cmath>
#include <vector>
#include "imageio/RectLandmark.hpp"

class Annotations {
public:
    Annotations() = default;
    explicit Annotations(const std::vector<imageio::RectLandmark>& landmarks, cv::Size minSize = cv::Size()) {
        for (const auto& landmark : landmarks) {
            const cv::Rect bounds = getBounds(landmark);
            nonNegatives.push_back(bounds);
            if (isFuzzy(landmark, bounds, minSize)) fuzzies.push_back(bounds);
            else positives.push_back(bounds);
        }
    }
    std::vector<cv::Rect> nonNegatives;   // positives and fuzzies
    std::vector<cv::Rect> positives;
    std::vector<cv::Rect> fuzzies;        // neither positive nor negative
private:
    static cv::Rect getBounds(const imageio::RectLandmark& landmark) {   // the float corners, each rounded half away from zero
        const cv::Rect_<float> rect = landmark.getRect();
        const int x = static_cast<int>(std::round(rect.x)), y = static_cast<int>(std::round(rect.y));
        const int width = static_cast<int>(std::round(rect.x + rect.width)) - x, height = static_cast<int>(std::round(rect.y + rect.height)) - y;
        return cv::Rect(x, y, width, height);
    }
    static bool isFuzzy(const imageio::RectLandmark& landmark, cv::Rect bounds, cv::Size minSize) {
        return landmark.getName().compare(0, 6, "ignore") == 0 || (bounds.width < minSize.width && bounds.height < minSize.height);
    }
};
