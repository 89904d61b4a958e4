// TEST INFRASTRUCTURE ONLY: a stand-in for the sliver of <opencv2/core/core.hpp> that the reference's vendored DBoW2 uses, so
// that its sources compile unmodified and in place into oracle/_ref/ref_dbow2 (see ../ref_dbow2.cpp). Written from scratch
// against the call sites: a reference-counted byte matrix (create / zeros / clone / release / ptr<T> / rows / cols / empty,
// shallow copies like cv::Mat's), the two type codes, and FileStorage / FileNode shells for two virtual members of
// TemplatedVocabulary that the driver never calls (every one of their members aborts).
#ifndef REF_DBOW2_OPENCV_STANDIN_HPP
#define REF_DBOW2_OPENCV_STANDIN_HPP

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#define CV_8U 0
#define CV_32F 5

namespace cv {

class Mat {
public:
    int rows, cols;
    Mat() : rows(0), cols(0), type_(CV_8U) {}
    void create(int r, int c, int type) {
        if (buf_ && r == rows && c == cols && type == type_) return;   // same shape: the buffer is kept, as cv::Mat does
        rows = r; cols = c; type_ = type;
        buf_ = std::make_shared<std::vector<unsigned char> >((size_t)r * (size_t)c * (type == CV_32F ? 4 : 1));
    }
    static Mat zeros(int r, int c, int type) { Mat m; m.create(r, c, type); return m; }   // a fresh vector is zero-filled
    Mat clone() const {
        Mat m;
        if (buf_) { m.create(rows, cols, type_); *m.buf_ = *buf_; }
        return m;
    }
    void release() { buf_.reset(); rows = cols = 0; }
    bool empty() const { return !buf_ || buf_->empty(); }
    template <class T> T* ptr(int row = 0) { return buf_ ? reinterpret_cast<T*>(buf_->data()) + (size_t)row * cols : NULL; }
    template <class T> const T* ptr(int row = 0) const { return buf_ ? reinterpret_cast<const T*>(buf_->data()) + (size_t)row * cols : NULL; }

private:
    int type_;
    std::shared_ptr<std::vector<unsigned char> > buf_;
};

inline void standin_unreachable(const char* what) {
    std::fprintf(stderr, "ref_dbow2: the OpenCV stand-in does not implement %s\n", what);
    std::abort();
}

class FileNode {
public:
    FileNode operator[](const std::string&) const { standin_unreachable("FileNode[]"); return FileNode(); }
    FileNode operator[](const char*) const { standin_unreachable("FileNode[]"); return FileNode(); }
    FileNode operator[](int) const { standin_unreachable("FileNode[]"); return FileNode(); }
    FileNode operator[](unsigned int) const { standin_unreachable("FileNode[]"); return FileNode(); }
    size_t size() const { standin_unreachable("FileNode::size"); return 0; }
    operator int() const { standin_unreachable("FileNode -> int"); return 0; }
    operator double() const { standin_unreachable("FileNode -> double"); return 0; }
    operator std::string() const { standin_unreachable("FileNode -> string"); return std::string(); }
};

class FileStorage {
public:
    enum { READ = 0, WRITE = 1 };
    FileStorage(const std::string&, int) { standin_unreachable("FileStorage"); }
    bool isOpened() const { return false; }
    FileNode operator[](const std::string&) const { standin_unreachable("FileStorage[]"); return FileNode(); }
};

template <class T> inline FileStorage& operator<<(FileStorage& fs, const T&) { standin_unreachable("FileStorage <<"); return fs; }

}  // namespace cv

#endif
