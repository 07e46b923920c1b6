// filtering_eval_app -- condensation::FilteringClassifierModel and ClassificationBasedStateValidator frame by frame on given samples and
// targets, so that a test can follow what the filter does to every sample and which candidates the validator asks.
//   usage: filtering_eval_app <config.cfg> <script.txt>
// config (boost info format):
//   tracking {
//     measurement positionDependent {                                        (the keys of tracking_setup.hpp)
//       feature hog|... { ... }
//       classifier { classifierFile <svm.txt> }                              (a stored ProbabilisticSvmClassifier: the inner model's classifier)
//       filter before { classifierFile <FDRVM1 file> [numFiltersToUse n] feature grayscale|h|whi { ... } }
//       wrapped 0                                                            (1: every extractor behind a PatchResizingFeatureExtractor(.., 1):
//     }                                                                       the per-sample routes)
//     validator rvm { classifierFile .. feature .. { ... } sizes "0.5 1" displacements "-0.25 0 0.25" }      (optional)
//   }
// Whatever the filter key says (before or after), the app builds three models on the same extractors and classifiers: FilteringClassifierModel
// with RESET_WEIGHT (`before`), with KEEP_WEIGHT (`after`) and the plain SingleClassifierModel (`none`).
// script (plain text), per frame:
//   frame <image.pgm|ppm> <targetX> <targetY> <targetSize> <sampleCount>
//   <x> <y> <size>                                                            (sampleCount lines)
// Per frame the app prints
//   frame <f>
//   e <before target> <before weight %.17g> <after target> <after weight> <none target> <none weight>       (per sample)
//   validator <0|1> candidates <n>, then n lines "c <x> <y> <size>"           (with a validator block)
// and at the end
//   counters before fused <n> loop <n> after fused <n> loop <n> validator fused <n> loop <n>
#include <cstdio>
#include <fstream>
#include <iostream>
#include "tracking_setup.hpp"

using namespace imageprocessing;
using namespace classification;
using namespace condensation;
using boost::property_tree::ptree;
using std::make_shared;
using std::shared_ptr;
using std::string;

static cv::Mat read_pnm(const string& path) {
    std::ifstream f(path.c_str(), std::ios::binary);
    if (!f.is_open()) throw std::runtime_error("cannot open image " + path);
    string magic;
    int w, h, maxv;
    f >> magic >> w >> h >> maxv;
    f.get();
    if ((magic != "P5" && magic != "P6") || maxv != 255) throw std::runtime_error("only binary PGM/PPM with maxval 255 are supported");
    const int ch = magic == "P6" ? 3 : 1;
    cv::Mat img(h, w, CV_MAKETYPE(CV_8U, ch));
    f.read((char*)img.data, (size_t)w * h * ch);
    if (ch == 3)
        for (size_t i = 0; i < (size_t)w * h; ++i) std::swap(img.data[3 * i], img.data[3 * i + 2]);
    return img;
}

static shared_ptr<FeatureExtractor> maybe_wrapped(shared_ptr<FeatureExtractor> extractor, bool wrapped) {
    if (!wrapped) return extractor;
    return make_shared<PatchResizingFeatureExtractor>(extractor, 1.0);
}

int main(int argc, char** argv) {
    try {
        if (argc != 3) {
            std::fprintf(stderr, "usage: %s <config.cfg> <script.txt>\n", argv[0]);
            return 2;
        }
        ptree all;
        boost::property_tree::read_info(string(argv[1]), all);
        const ptree& pt = all.get_child("tracking");
        if (pt.get("measurement", string()) != "positionDependent") throw std::invalid_argument("the config needs a `measurement positionDependent` block");
        const ptree& mt = pt.get_child("measurement");
        FilteringClassifierModel::Behavior behavior;
        if (!tracking_setup::filterBehavior(mt, behavior)) throw std::invalid_argument("the config needs a `filter before|after { ... }` block");
        const bool wrapped = mt.get("wrapped", 0) != 0;
        shared_ptr<FeatureExtractor> extractor = maybe_wrapped(tracking_setup::createFeatureExtractor(mt.get_child("feature")), wrapped);
        shared_ptr<FeatureExtractor> filterExtractor = maybe_wrapped(tracking_setup::createFeatureExtractor(mt.get_child("filter.feature")), wrapped);
        shared_ptr<ProbabilisticSvmClassifier> classifier = ProbabilisticSvmClassifier::load(mt.get_child("classifier"));
        shared_ptr<RvmClassifier> filter = tracking_setup::createRvm(mt.get_child("filter"));
        FilteringClassifierModel before(filterExtractor, filter, extractor, classifier, FilteringClassifierModel::Behavior::RESET_WEIGHT);
        FilteringClassifierModel after(filterExtractor, filter, extractor, classifier, FilteringClassifierModel::Behavior::KEEP_WEIGHT);
        SingleClassifierModel none(extractor, classifier);
        shared_ptr<ClassificationBasedStateValidator> validator;
        if (pt.get("validator", string("none")) != "none") {
            const ptree& vt = pt.get_child("validator");
            validator = make_shared<ClassificationBasedStateValidator>(maybe_wrapped(tracking_setup::createFeatureExtractor(vt.get_child("feature")), wrapped),
                                                                       tracking_setup::createRvm(vt), tracking_setup::readValues(vt.get("sizes", string("1"))),
                                                                       tracking_setup::readValues(vt.get("displacements", string("0"))));
        }
        std::ifstream script(argv[2]);
        if (!script.is_open()) throw std::runtime_error(string("cannot open ") + argv[2]);
        auto image = make_shared<VersionedImage>();
        string word, path;
        int frame = 0;
        while (script >> word) {
            if (word != "frame") throw std::runtime_error("script: expected `frame`, got " + word);
            int tx, ty, ts, count;
            if (!(script >> path >> tx >> ty >> ts >> count) || count < 0) throw std::runtime_error("script: bad frame line");
            std::vector<std::vector<shared_ptr<Sample>>> sets(3);
            for (int i = 0; i < count; ++i) {
                int x, y, size;
                if (!(script >> x >> y >> size)) throw std::runtime_error("script: bad sample line");
                for (auto& set : sets) set.push_back(make_shared<Sample>(x, y, size));
            }
            image->setData(read_pnm(path));
            before.evaluate(image, sets[0]);
            after.evaluate(image, sets[1]);
            none.evaluate(image, sets[2]);
            std::printf("frame %d\n", frame);
            for (int i = 0; i < count; ++i)
                std::printf("e %d %.17g %d %.17g %d %.17g\n", sets[0][i]->isTarget() ? 1 : 0, sets[0][i]->getWeight(), sets[1][i]->isTarget() ? 1 : 0,
                            sets[1][i]->getWeight(), sets[2][i]->isTarget() ? 1 : 0, sets[2][i]->getWeight());
            if (validator) {
                const bool valid = validator->isValid(Sample(tx, ty, ts), sets[2], image);
                std::printf("validator %d candidates %zu\n", valid ? 1 : 0, validator->getLastCandidates().size());
                for (const cv::Rect& c : validator->getLastCandidates()) std::printf("c %d %d %d\n", c.x, c.y, c.width);
            }
            ++frame;
        }
        std::printf("counters before fused %d loop %d after fused %d loop %d validator fused %d loop %d\n", before.getFusedFilterCount(), before.getLoopFilterCount(),
                    after.getFusedFilterCount(), after.getLoopFilterCount(), validator ? validator->getFusedValidationCount() : 0,
                    validator ? validator->getLoopValidationCount() : 0);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "filtering_eval_app: %s\n", e.what());
        return 1;
    }
}
