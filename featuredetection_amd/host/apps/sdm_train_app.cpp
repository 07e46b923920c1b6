// sdm_train_app -- the reference's sdmTraining app (sdmTraining.cpp:172-270,455-461) on this backend: from annotated images to a model
// file that sdm_fit_app --non-adaptive reads.
//   sdm_train_app <images.lst> <training.cfg> <out-model.txt> [--seed N] [--trace file] [--prepare-only]
// images.lst: one line per image, `image.pgm x y w h landmarks.txt` -- a binary PGM, the face box (given: the reference's Viola-Jones
// call is OpenCV's and stays out) and a landmark file with `name x y` per line, as imageio::SimpleModelLandmarkSink writes.
// training.cfg: the reference's INFO format: parameters.{numSamplesPerImage, numCascadeSteps, regularisationFactor,
// regulariseAffineComponent, regulariseWithEigenvalueThreshold, featureDescriptors.*} and modelLandmarks.landmarks (the names, in
// model order).  --seed: the seed of the perturbed start shapes (default 5489).  --trace: a JSON record of the preparation (mean
// after every stage, both alignment statistics, every drawn (scale, tx, ty), the start shapes) and, after training, lambda and the
// two errors per step, R per step and the final shapes in the order of images.lst.  --prepare-only: stop after the preparation; no
// device is touched and no model is written.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include "fdcompat/ptree.hpp"
#include "superviseddescent/LandmarkBasedSupervisedDescentTraining.hpp"

using namespace superviseddescent;
using std::string;
using std::vector;
using Training = LandmarkBasedSupervisedDescentTraining;

static cv::Mat readPgm(const string& path) {
    std::ifstream f(path, std::ios::binary);
    string magic;
    int w = 0, h = 0, maxv = 0;
    f >> magic >> w >> h >> maxv;
    f.get();
    if (!f || magic != "P5" || maxv != 255 || w < 1 || h < 1) throw std::runtime_error("need a binary PGM: " + path);
    cv::Mat img(h, w, CV_8UC1);
    f.read((char*)img.data, (size_t)w * h);
    if (!f) throw std::runtime_error("truncated PGM: " + path);
    return img;
}

static void writeFloats(std::ostream& o, const char* key, const vector<float>& v, bool comma = true) {
    o << "\"" << key << "\": [";
    char buf[32];
    for (size_t i = 0; i < v.size(); ++i) { std::snprintf(buf, sizeof(buf), "%.9g", v[i]); o << (i ? ", " : "") << buf; }
    o << "]" << (comma ? ",\n" : "\n");
}
static void writeStats(std::ostream& o, const char* key, const Training::AlignmentStatistics& s) {
    writeFloats(o, key, {s.tx.mu, s.tx.sigma, s.ty.mu, s.ty.sigma, s.sx.mu, s.sx.sigma, s.sy.mu, s.sy.sigma});
}

int main(int argc, char** argv) {
    try {
        vector<string> pos;
        unsigned int seed = 5489u;
        string tracePath;
        bool prepareOnly = false;
        for (int a = 1; a < argc; ++a) {
            const string arg = argv[a];
            if (arg == "--seed" && a + 1 < argc) seed = (unsigned int)std::strtoul(argv[++a], nullptr, 10);
            else if (arg == "--trace" && a + 1 < argc) tracePath = argv[++a];
            else if (arg == "--prepare-only") prepareOnly = true;
            else pos.push_back(arg);
        }
        if (pos.size() != 3) {
            std::fprintf(stderr, "call: %s images.lst training.cfg out-model.txt [--seed N] [--trace file] [--prepare-only]\n", argv[0]);
            return 2;
        }
        boost::property_tree::ptree pt;
        boost::property_tree::read_info(pos[1], pt);
        const auto& par = pt.get_child("parameters");
        Training::Regularisation reg;
        const int numSamples = par.get<int>("numSamplesPerImage", 10), numSteps = par.get<int>("numCascadeSteps", 5);
        reg.factor = par.get<float>("regularisationFactor", 0.5f);
        reg.regulariseAffineComponent = par.get<int>("regulariseAffineComponent", 0) != 0;
        reg.regulariseWithEigenvalueThreshold = par.get<int>("regulariseWithEigenvalueThreshold", 0) != 0;
        vector<string> descriptorTypes;
        vector<std::shared_ptr<DescriptorExtractor>> extractors;
        for (const auto& kv : par.get_child("featureDescriptors")) {   // sdmTraining.cpp:194-230
            const string type = kv.second.get<string>("descriptorType");
            std::istringstream ps(kv.second.get<string>("descriptorParameters", string()));
            string k1, k2, k3;
            int numCells = 0, cellSize = 0, numBins = 0;
            ps >> k1 >> numCells >> k2 >> cellSize >> k3 >> numBins;
            if (type != "vlhog-dt" && type != "vlhog-uoctti")
                throw std::logic_error("descriptorType does not match 'vlhog-dt' or 'vlhog-uoctti' (OpenCVSift is not available on this backend).");
            if (!ps || k1 != "numCells" || k2 != "cellSize" || k3 != "numBins")
                throw std::logic_error("descriptorParameters must contain numCells, cellSize and numBins.");
            extractors.push_back(std::make_shared<VlHogDescriptorExtractor>(
                type == "vlhog-dt" ? VlHogDescriptorExtractor::VlHogType::DalalTriggs : VlHogDescriptorExtractor::VlHogType::Uoctti, numCells, cellSize, numBins));
            descriptorTypes.push_back(type);
        }
        vector<string> modelLandmarks;
        for (const auto& kv : pt.get_child("modelLandmarks").get_child("landmarks")) modelLandmarks.push_back(kv.first);
        if (modelLandmarks.empty()) throw std::runtime_error("modelLandmarks.landmarks is empty");
        const int L = (int)modelLandmarks.size();

        vector<cv::Mat> images, landmarks;
        vector<cv::Rect> boxes;
        std::ifstream lst(pos[0]);
        if (!lst.is_open()) throw std::runtime_error("cannot open " + pos[0]);
        string line;
        while (std::getline(lst, line)) {
            std::istringstream ls(line);
            string img, lmFile;
            int x, y, w, h;
            if (!(ls >> img >> x >> y >> w >> h >> lmFile)) continue;
            images.push_back(readPgm(img));
            boxes.push_back(cv::Rect(x, y, w, h));
            std::map<string, std::pair<float, float>> byName;
            std::ifstream lf(lmFile);
            if (!lf.is_open()) throw std::runtime_error("cannot open " + lmFile);
            string name;
            float px, py;
            while (lf >> name >> px >> py) byName[name] = std::make_pair(px, py);
            cv::Mat row(1, 2 * L, CV_32FC1);
            for (int i = 0; i < L; ++i) {
                auto it = byName.find(modelLandmarks[i]);
                if (it == byName.end()) throw std::runtime_error(lmFile + " has no landmark " + modelLandmarks[i]);
                row.at<float>(0, i) = it->second.first;
                row.at<float>(0, i + L) = it->second.second;
            }
            landmarks.push_back(row);
        }
        if (images.empty()) throw std::runtime_error("no training images in " + pos[0]);

        Training tr(seed);
        tr.setNumSamplesPerImage(numSamples);
        tr.setNumCascadeSteps(numSteps);
        tr.setRegularisation(reg);
        tr.setAlignGroundtruth(Training::AlignGroundtruth::NONE);                       // sdmTraining.cpp:458-459
        tr.setMeanNormalization(Training::MeanNormalization::UNIT_SUM_SQUARED_NORMS);
        tr.setPrepareOnly(prepareOnly);
        SdmLandmarkModel model = tr.train(images, landmarks, boxes, modelLandmarks, descriptorTypes, extractors);
        if (!prepareOnly) model.save(pos[2], "trained by sdm_train_app");
        if (!tracePath.empty()) {
            const Training::Trace& t = tr.getTrace();
            std::ofstream o(tracePath);
            o << "{\n\"images\": " << images.size() << ", \"samples\": " << numSamples + 1 << ", \"landmarks\": " << L << ", \"seed\": " << seed << ",\n";
            writeFloats(o, "mean", t.mean);
            writeFloats(o, "normalised_mean", t.normalisedMean);
            writeStats(o, "alignment_statistics_1", t.first);
            writeFloats(o, "rescaled_mean", t.rescaledMean);
            writeStats(o, "alignment_statistics_2", t.second);
            writeFloats(o, "draws", t.draws);
            o << "\"steps\": [";
            char buf[160];
            for (size_t s = 0; s < t.steps.size(); ++s) {
                std::snprintf(buf, sizeof(buf), "%s{\"lambda\": %.17g, \"err_l1\": %.17g, \"err_fro\": %.17g, \"dim\": %d}", s ? ", " : "", t.steps[s].lambda,
                              t.steps[s].err_l1, t.steps[s].err_fro, t.steps[s].dim);
                o << buf;
            }
            o << "],\n\"R\": [";
            for (int s = 0; s < model.getNumCascadeSteps(); ++s) {
                cv::Mat R = model.getRegressorData(s);
                vector<float> v((size_t)R.rows * R.cols);
                for (int r = 0; r < R.rows; ++r) for (int c = 0; c < R.cols; ++c) v[(size_t)r * R.cols + c] = R.at<float>(r, c);
                std::ostringstream one;
                writeFloats(one, "x", v, false);
                const string js = one.str();
                o << (s ? ", " : "") << js.substr(js.find('['), js.rfind(']') - js.find('[') + 1);
            }
            o << "],\n";
            writeFloats(o, "final_shapes", t.finalShapes);
            writeFloats(o, "start_shapes", t.startShapes, false);
            o << "}\n";
        }
        if (!prepareOnly) {
            const auto& st = tr.getTrace().steps;
            for (size_t s = 0; s < st.size(); ++s) std::printf("step %zu: lambda %.9g  L1 %.6f  Frobenius %.6f\n", s, st[s].lambda, st[s].err_l1, st[s].err_fro);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
