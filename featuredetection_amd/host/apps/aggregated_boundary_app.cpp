// aggregated_boundary_app -- where the host layer's approximated feature pyramid ends: every composition this backend does not build
// must fail with std::logic_error instead of computing something else.  Prints one line per case, "<case> <what happened>", and
// returns 0 when every case ended in logic_error.
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include "detection/detection_all.hpp"
#include "imageprocessing/extraction/AggregatedFeaturesExtractor.hpp"
#include "imageprocessing/filtering/FhogFilter.hpp"

using namespace imageprocessing;
using imageprocessing::extraction::AggregatedFeaturesExtractor;
using imageprocessing::filtering::FhogFilter;
using std::make_shared;

static bool expect_logic_error(const char* name, const std::function<void()>& body) {
    const char* outcome = "no_exception";
    try { body(); }
    catch (const std::logic_error& e) {   // invalid_argument is a logic_error too: tell them apart
        outcome = dynamic_cast<const std::invalid_argument*>(&e) ? "invalid_argument" : "logic_error";
    }
    catch (const std::exception&) { outcome = "other_exception"; }
    std::printf("%s %s\n", name, outcome);
    return std::string(outcome) == "logic_error";
}

int main() {
    bool ok = true;
    cv::Mat image(120, 160, CV_8UC1);
    std::memset(image.data, 7, (size_t)120 * 160);
    auto approximated = [] {
        auto p = ImagePyramid::createApproximated(4, 0.5, 1.0);
        p->addImageFilter(make_shared<GrayscaleFilter>());
        p->addLayerFilter(make_shared<FhogFilter>(8, 9, false, true, 0.2f));
        return p;
    };
    ok &= expect_logic_error("approximate_a_source_pyramid", [&] { ImagePyramid::createApproximated(make_shared<ImagePyramid>((size_t)1, 0.5, 1.0), 4); });
    ok &= expect_logic_error("update", [&] { approximated()->update(image); });
    ok &= expect_logic_error("get_layers", [&] { approximated()->getLayers(); });
    ok &= expect_logic_error("layer_scales", [&] { approximated()->getLayerScales(); });
    ok &= expect_logic_error("other_layer_filter", [&] { ImagePyramid::createApproximated(4, 0.5, 1.0)->addLayerFilter(make_shared<LbpFilter>(LbpFilter::Type::LBP8)); });
    ok &= expect_logic_error("second_layer_filter", [&] { approximated()->addLayerFilter(make_shared<FhogFilter>(8, 9, false, true, 0.2f)); });
    ok &= expect_logic_error("sliding_window_extractor", [&] { DirectPyramidFeatureExtractor(approximated(), 20, 20).update(image); });
    ok &= expect_logic_error("extractor_on_exact_pyramid",
                             [&] { AggregatedFeaturesExtractor(make_shared<ImagePyramid>((size_t)4, 0.5, 1.0), cv::Size(8, 8), 8, true, 0); });
    ok &= expect_logic_error("fixed_min_scale", [&] { AggregatedFeaturesExtractor(approximated(), cv::Size(8, 8), 8, false, 0); });
    return ok ? 0 : 1;
}
