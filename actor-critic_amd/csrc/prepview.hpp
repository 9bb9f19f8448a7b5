// The prepared-weight buffer (net->conv_prep, acmi_conv_prep_bytes(C3) bytes, written
// by acmi_conv_prepare), host side only:
//   [tower fragments | bounds header | conv2^T | fc4 | conv3^T]
//    tower.hpp TowerPrep<C3> .......   convt2.hpp CT2   fc4roll.hpp   convt3.hpp CT3Prep<C3>
// Every section's offset is here and nowhere else; the kernels receive the
// section pointers.  A null base ("no prepared weights") gives null members.
#pragma once

#include "convt2.hpp"
#include "convt3.hpp"
#include "fc4roll.hpp"
#include "tower.hpp"

namespace acmi {

template <int C3>
struct PrepView {
  char* base;  // (acmi_conv_prepare writes through the view; every other caller reads)
  explicit PrepView(const void* prep) : base(static_cast<char*>(const_cast<void*>(prep))) {}
  static long long ct2_off() { return TowerPrep<C3>::BYTES; }
  static long long fc4_off() { return ct2_off() + CT2::BYTES; }
  static long long ct3_off() { return fc4_off() + fc4_prep_bytes(49 * C3); }
  static long long bytes() { return ct3_off() + CT3Prep<C3>::BYTES; }
  char* at(long long off) const { return base ? base + off : nullptr; }
  char* tower() const { return base; }
  // the header's eight published bounds; bound(kTowMaxW3 ...): one of them
  unsigned* hdr() const { return reinterpret_cast<unsigned*>(at(TowerPrep<C3>::HDR)); }
  unsigned* bound(int word) const { return base ? hdr() + word : nullptr; }
  char* ct2() const { return at(ct2_off()); }
  char* fc4() const { return at(fc4_off()); }
  char* ct3() const { return at(ct3_off()); }
};

}  // namespace acmi
