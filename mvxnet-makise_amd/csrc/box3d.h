// The oriented 3-D box of the point-in-box decisions (GT database crop, per-object augmentation): f64, one operand order.
#pragma once
#include "common.h"

struct Box { double x, y, z, hl, hw, h, c, s; };                 // centre (z = bottom face), half length / width, height, cos / sin of the yaw

// b3 = [x y z l w h ...] in f32; (c, s) = cos and sin of the yaw, as the caller has them
__device__ __forceinline__ Box load_box(const float *b3, double c, double s) {
    Box b;
    b.x = (double)b3[0]; b.y = (double)b3[1]; b.z = (double)b3[2];
    b.hl = (double)b3[3] / 2.0; b.hw = (double)b3[4] / 2.0; b.h = (double)b3[5];
    b.c = c; b.s = s;
    return b;
}

// (u, v): the point in the box frame, the inverse of Calc.bbox3d2bev's corner @ [[c, -s], [s, c]] + (x, y);
// |u| <= l/2, |v| <= w/2, 0 <= dz <= h
__device__ __forceinline__ bool inside(const Box &b, double x, double y, double z) {
    const double dx = x - b.x, dy = y - b.y, dz = z - b.z;
    const double u = dx * b.c - dy * b.s, v = dx * b.s + dy * b.c;
    return fabs(u) <= b.hl && fabs(v) <= b.hw && dz >= 0.0 && dz <= b.h;
}
