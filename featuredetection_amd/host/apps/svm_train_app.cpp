// svm_train_app -- trains a libsvm::LibSvmClassifier on a feature matrix the way headTrackingApp configures one (HeadTracking.cpp:
// 330-360, default.cfg:133-153): a binary C-SVC, optionally with libsvm's sigmoid fit, or a one-class SVM.
//   svm_train_app <features.txt> <classifier.cfg> <out-svm.txt> [--seed N]
// features.txt: `positives negatives dimensions` on the first line, then one example per line, the positives first (no negatives
// are read for one-class training).
// classifier.cfg: the reference's INFO format with headTrackingApp's keys:
//   kernel rbf        ; rbf | poly | hik | linear
//   { gamma 0.1  alpha 0.05  constant 0  degree 2 }
//   training binary   ; binary | one-class | liblinear
//   { C 1  nu 0.5  compensateImbalance false  probabilistic false }
// `training liblinear { C 1  bias false  staticNegativeExamples true { filename f  amount n  scale s } }` trains a
// liblinear::LibLinearClassifier the way headTrackingApp's `classifier libLinear` does (HeadTracking.cpp:368-385); the kernel has
// to be linear.  It prints the bias, the iterations and the CG steps.
// --seed: std::srand's seed (default 1, the C library's own), which decides the shuffle of the sigmoid fit's five folds.
// Writes the SvmClassifier text format, followed by the `Logistic a b` line when probabilistic (a = libsvm's probB, b = probA), and
// prints rho, the number of support vectors and, when probabilistic, probA and probB with 17 digits.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include "fdcompat/ptree.hpp"
#include "liblinear/LibLinearClassifier.hpp"
#include "libsvm/LibSvmClassifier.hpp"

using namespace classification;
using std::string;
using std::vector;

static bool flag(const boost::property_tree::ptree& node, const string& key) {
    const string v = node.get<string>(key, "false");
    return v == "true" || v == "1";
}

int main(int argc, char** argv) {
    try {
        vector<string> pos;
        unsigned int seed = 1u;
        for (int a = 1; a < argc; ++a) {
            const string arg = argv[a];
            if (arg == "--seed" && a + 1 < argc) seed = (unsigned int)std::strtoul(argv[++a], nullptr, 10);
            else pos.push_back(arg);
        }
        if (pos.size() != 3) {
            std::fprintf(stderr, "call: %s features.txt classifier.cfg out-svm.txt [--seed N]\n", argv[0]);
            return 2;
        }
        boost::property_tree::ptree pt;
        boost::property_tree::read_info(pos[1], pt);
        const string kernelType = pt.get<string>("kernel");
        const boost::property_tree::ptree& kp = pt.get_child("kernel");
        std::shared_ptr<Kernel> kernel;
        if (kernelType == "rbf") kernel.reset(new RbfKernel(kp.get<double>("gamma")));
        else if (kernelType == "poly") kernel.reset(new PolynomialKernel(kp.get<double>("alpha"), kp.get<double>("constant"), kp.get<int>("degree")));
        else if (kernelType == "hik") kernel.reset(new HistogramIntersectionKernel());
        else if (kernelType == "linear") kernel.reset(new LinearKernel());
        else throw std::invalid_argument("invalid kernel type: " + kernelType);
        const string trainingType = pt.get<string>("training");
        const boost::property_tree::ptree& tp = pt.get_child("training");
        const bool oneClass = trainingType == "one-class";
        const bool libLinear = trainingType == "liblinear";
        if (libLinear && kernelType != "linear") throw std::invalid_argument("training liblinear needs kernel linear, not " + kernelType);
        if (!oneClass && !libLinear && trainingType != "binary") throw std::invalid_argument("invalid training type: " + trainingType);
        const bool probabilistic = !oneClass && flag(tp, "probabilistic");

        std::ifstream in(pos[0]);
        if (!in.is_open()) throw std::runtime_error("cannot open " + pos[0]);
        int positives = 0, negatives = 0, dimensions = 0;
        in >> positives >> negatives >> dimensions;
        if (!in || positives < 1 || negatives < 0 || dimensions < 1) throw std::runtime_error("need `positives negatives dimensions` first: " + pos[0]);
        vector<cv::Mat> positiveExamples, negativeExamples;
        for (int i = 0; i < positives + (oneClass ? 0 : negatives); ++i) {
            cv::Mat row(1, dimensions, CV_32FC1);
            for (int k = 0; k < dimensions; ++k) in >> row.at<float>(0, k);
            (i < positives ? positiveExamples : negativeExamples).push_back(row);
        }
        if (!in) throw std::runtime_error("truncated feature matrix: " + pos[0]);

        if (libLinear) {
            liblinear::LibLinearClassifier trainer(tp.get<double>("C", 1.0), flag(tp, "bias"));
            if (tp.count("staticNegativeExamples") && flag(tp, "staticNegativeExamples")) {
                const boost::property_tree::ptree& np = tp.get_child("staticNegativeExamples");
                trainer.loadStaticNegatives(np.get<string>("filename"), np.get<int>("amount"), np.get<double>("scale"));
            }
            if (!trainer.retrain(positiveExamples, negativeExamples)) throw std::runtime_error("the classifier is not usable after the training");
            const fd_liblinear_info& info = trainer.getLastTrainingInfo();
            std::printf("bias %.9g\niterations %d\ncg_steps %d\nnegatives %d\n", trainer.getSvm()->getBias(), info.iterations, info.cg_steps,
                        trainer.getLastNegativeCount());
            std::ofstream out(pos[2]);
            if (!out.is_open()) throw std::runtime_error("cannot write " + pos[2]);
            trainer.getSvm()->store(out);
            return 0;
        }
        std::shared_ptr<libsvm::LibSvmClassifier> trainer =
            oneClass ? libsvm::LibSvmClassifier::createOneClassKernelSvm(kernel, tp.get<double>("nu", 0.5))
                     : libsvm::LibSvmClassifier::createBinaryKernelSvm(kernel, tp.get<double>("C", 1.0), flag(tp, "compensateImbalance"), probabilistic);
        std::srand(seed);
        if (!trainer->retrain(positiveExamples, negativeExamples)) throw std::runtime_error("the classifier is not usable after the training");
        const fd_svm_train_info& info = trainer->getLastTrainingInfo();
        std::printf("rho %.17g\nn_sv %d\niterations %d\n", info.rho, info.n_sv, info.iterations);
        if (probabilistic) std::printf("probA %.17g\nprobB %.17g\n", trainer->getLastProbA(), trainer->getLastProbB());
        std::ofstream out(pos[2]);
        if (!out.is_open()) throw std::runtime_error("cannot write " + pos[2]);
        if (probabilistic) trainer->getProbabilisticSvm()->store(out);
        else trainer->getSvm()->store(out);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
