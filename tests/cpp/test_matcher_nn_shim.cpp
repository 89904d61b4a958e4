// The tracking line test_vo_1 runs (reference test/test_vo.cpp:213), Matcher::searchByNN(cur, key_frame, 0, 5, 10, 30), on the
// header shims: two images, ORB, the matcher with the reference's arguments and with a second seed, and the calls the reference
// leaves undefined (a level sub-range, MapPointOnly). Every result goes to a binary file that tests/test_gpu_shim_nn.py compares
// with the C ABI's own list.
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <vector>

#include "camera/CameraModel.h"
#include "extractors/ORBextractor.h"
#include "matchers/matcher.h"
#include "types/Frame.h"

using namespace TRACKING_BENCH;

static cv::Mat read_pgm(const char* path)
{
    std::ifstream f(path, std::ios::binary);
    std::string magic; int w, h, maxv;
    f >> magic >> w >> h >> maxv;
    f.get();
    cv::Mat m(h, w, CV_8UC1);
    f.read((char*)m.data, (std::streamsize)w * h);
    if (!f || magic != "P5") { std::cerr << "cannot read " << path << std::endl; std::exit(2); }
    return m;
}
template <typename T> static void put(std::ofstream& o, const T* p, size_t n) { int32_t c = (int32_t)n; o.write((char*)&c, 4); o.write((const char*)p, (std::streamsize)(n * sizeof(T))); }

int main(int argc, char** argv)
{
    if (argc < 4) { std::cerr << "usage: test_matcher_nn_shim left.pgm right.pgm out.bin" << std::endl; return 2; }
    cv::Mat img1 = read_pgm(argv[1]), img2 = read_pgm(argv[2]);
    auto camera_ptr = std::make_shared<PinholeCamera>(img1.cols, img1.rows, 718.856f, 718.856f, 607.1928f, 185.2157f);
    auto frame1_ptr = std::make_shared<Frame>(img1, 0, 5, 0.8, camera_ptr);
    auto frame2_ptr = std::make_shared<Frame>(img2, 0, 5, 0.8, camera_ptr);
    auto extractor_ptr = std::make_shared<ORBExtractor>();
    std::vector<cv::KeyPoint> keypoints1, keypoints2;
    cv::Mat descriptors1, descriptors2;
    extractor_ptr->operator()(frame1_ptr->GetImagePyramid(), frame1_ptr->GetScaleFactors(), 1000, 80, 30, keypoints1, descriptors1);
    frame1_ptr->SetKeys(keypoints1, frame1_ptr, descriptors1);
    extractor_ptr->operator()(frame2_ptr->GetImagePyramid(), frame2_ptr->GetScaleFactors(), 1000, 80, 30, keypoints2, descriptors2);
    frame2_ptr->SetKeys(keypoints2, frame2_ptr, descriptors2);

    auto matcher_ptr = std::make_shared<Matcher>();
    auto matches = matcher_ptr->searchByNN(frame1_ptr, frame2_ptr, 0, 5, 10, 30);
    auto loose = matcher_ptr->searchByNN(frame1_ptr, frame2_ptr, 0, 5, 1000, 300);
    matcher_ptr->lsh_seed = 7;
    matcher_ptr->lsh_tables = 4; matcher_ptr->lsh_key_size = 16; matcher_ptr->lsh_multi_probe_level = 1;
    auto other = matcher_ptr->searchByNN(frame1_ptr, frame2_ptr, 0, 5, 1000, 300);

    // the branches the reference leaves undefined surface as searchByBF's do: std::invalid_argument
    int32_t refused[4] = {0, 0, 0, 0};
    try { matcher_ptr->searchByNN(frame1_ptr, frame2_ptr, 0, 4, 10, 30); } catch (const std::invalid_argument&) { refused[0] = 1; }
    try { matcher_ptr->searchByNN(frame1_ptr, frame2_ptr, 1, 5, 10, 30); } catch (const std::invalid_argument&) { refused[1] = 1; }
    try { matcher_ptr->searchByNN(frame1_ptr, frame2_ptr, 0, 5, 10, 30, true); } catch (const std::invalid_argument&) { refused[2] = 1; }
    try { matcher_ptr->searchByBF(frame1_ptr, frame2_ptr, 0, 4, 10, 30); } catch (const std::invalid_argument&) { refused[3] = 1; }

    std::ofstream o(argv[3], std::ios::binary);
    put(o, descriptors1.data, (size_t)descriptors1.rows * 32);
    put(o, descriptors2.data, (size_t)descriptors2.rows * 32);
    put(o, matches.data(), matches.size()); put(o, loose.data(), loose.size()); put(o, other.data(), other.size());
    put(o, refused, 4);
    std::cout << "kps " << keypoints1.size() << "/" << keypoints2.size() << " nn " << matches.size() << " loose " << loose.size()
              << " other " << other.size() << std::endl;
    return 0;
}
