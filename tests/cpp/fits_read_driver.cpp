// fits_read_driver.cpp -- reads an image with fits_read_mask (the reader behind SLICER_amd --pcl-mask) and writes its
// npix^2 f32 values, in the machine's byte order, to stdout; tests/test_pcl_host.py compares them with what
// slicer_amd.fits.write_image was given.  A refused file: the reason on stderr, exit status 1.
// usage: fits_read_driver <file.fits> <npix>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "fits_writer.hpp"

int main(int argc, char **argv)
{
    if (argc != 3)
        return 2;
    const int npix = atoi(argv[2]);
    if (npix < 1 || npix > 16384)
        return 2;
    std::vector<float> image((size_t)npix * (size_t)npix);
    const std::string why = slicer_amd::fits_read_mask(argv[1], npix, image.data());
    if (!why.empty()) {
        fprintf(stderr, "%s\n", why.c_str());
        return 1;
    }
    return fwrite(image.data(), sizeof(float), image.size(), stdout) == image.size() ? 0 : 3;
}
