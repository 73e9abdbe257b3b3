/*
 * odtk_conv_strided.h -- libodtk_conv.so on views: the convolution of include/odtk_conv.h with explicit element strides.
 * (A header of its own: odtk_conv.h is the surface tests/test_conv_library_host.py pins name by name.)
 */
#ifndef ODTK_CONV_STRIDED_H
#define ODTK_CONV_STRIDED_H

#include "odtk_conv.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * odtk_conv_bias_act_pads on VIEWS of larger channels_last buffers: element strides (image, row, pixel) for x and for y, the
 * channel stride stays 1.  odtk_conv_bias_act and odtk_conv_bias_act_pads forward here with the packed strides.  (The engine's
 * pyramid canvas, odtk/fused.py: the heads' last convolutions read their level's rectangle of the canvas in place.)
 *   - the strides of a tensor that is not packed must be multiples of 8 elements and its base 16-byte aligned (the instances'
 *     16-byte vector accesses); pixels must not overlap, rows must hold their pixels and images their rows: ODTK_ERR_INVALID
 *     otherwise;
 *   - x: any such view.  The instances' input descriptor carries all three strides;
 *   - y: the pixel stride is free (a channel slice of a wider tensor), but the rows and images must follow each other at that
 *     stride (row stride = out_w * pixel stride, image stride = out_h * row stride): the prebuilt instances address the output as
 *     ONE run of batch * out_h * out_w pixels, so a rectangle of a wider buffer is refused with ODTK_ERR_UNSUPPORTED -- the
 *     caller convolves into a packed tensor and copies;
 *   - plans stay keyed on the extents; the instance of the plan is asked (IsSupportedArgument, no workspace) about the actual
 *     strided argument once per (problem, strides) pair before its first launch: ODTK_ERR_UNSUPPORTED if it refuses.
 */
int odtk_conv_bias_act_strided(void *y, const void *x, const void *w, const void *bias, int batch_size, int c_in, int height, int width,
                               int c_out, int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int pad_h_end,
                               int pad_w_end, long long x_image_stride, long long x_row_stride, long long x_pixel_stride,
                               long long y_image_stride, long long y_row_stride, long long y_pixel_stride, int dtype, int relu,
                               void *stream);

#ifdef __cplusplus
}
#endif
#endif
