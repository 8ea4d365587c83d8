// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  Stand-in for cv::Mat as TextSLAM's cost-functor headers use it: a single-channel
// 8-bit image, continuous rows.  A Mat is a view (it never frees what it was given); clone() owns its copy.
#ifndef TSREF_SHIM_OPENCV_CORE
#define TSREF_SHIM_OPENCV_CORE
#include <cstddef>
#include <cstring>
#include <memory>
#include <stdint.h>
#include <vector>

namespace cv {

class Mat {
public:
    int rows, cols;
    unsigned char *data;
    Mat() : rows(0), cols(0), data(NULL), step_(0) {}
    Mat(int r, int c, unsigned char *d) : rows(r), cols(c), data(d), step_(c) {}
    Mat clone() const {
        Mat m; m.rows = rows; m.cols = cols; m.step_ = cols;
        m.own_ = std::make_shared<std::vector<unsigned char> >((size_t)rows*cols + 1);
        m.data = m.own_->data();
        for (int r = 0; r < rows; r++) std::memcpy(m.data + (size_t)r*cols, data + (size_t)r*step_, (size_t)cols);
        return m;
    }
    Mat row(int y) const { Mat m(*this); m.rows = 1; m.data = data + (size_t)y*step_; return m; }
    Mat col(int x) const { Mat m(*this); m.cols = 1; m.data = data + x; return m; }
    template <typename T> T *ptr(int y = 0) { return (T *)(data + (size_t)y*step_); }
    template <typename T> const T *ptr(int y = 0) const { return (const T *)(data + (size_t)y*step_); }
    template <typename T> T &at(int y, int x) { return ((T *)(data + (size_t)y*step_))[x]; }
    template <typename T> const T &at(int y, int x) const { return ((const T *)(data + (size_t)y*step_))[x]; }
private:
    int step_;
    std::shared_ptr<std::vector<unsigned char> > own_;
};

}  // namespace cv
#endif
