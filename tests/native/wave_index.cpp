// tests/native/wave_index.cpp -- host check of the decoder's workgroup-slot ->
// wave function (cuzfp::decode_wave_of in cuzfp_amd/csrc/wave_index.hpp).  For
// every launch size given on the command line (or a built-in list), workgroups
// of 8 and 16 waves against the encoder's 4, with the remap where
// decode_remap_ok allows it and without: the slots of ceil(nwaves / wpg)
// workgroups must hit every wave of [0, nwaves) exactly once and put every
// other (padding) slot at or past nwaves; under the remap a slot's wave must
// belong to an encoder workgroup of the decoder workgroup's own index mod 8.
// Prints the number of violations.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../cuzfp_amd/csrc/wave_index.hpp"

int main(int argc, char** argv) {
  std::vector<uint32_t> sizes;
  for (int i = 1; i < argc; i++) sizes.push_back((uint32_t)strtoul(argv[i], nullptr, 10));
  if (sizes.empty())
    for (uint32_t n = 1; n <= 700; n++) sizes.push_back(n);
  long bad = 0, remapped = 0;
  const uint32_t enc = 4;
  for (uint32_t wpg : {4u, 8u, 16u, 12u})
    for (uint32_t n : sizes)
      for (int want = 0; want < 2; want++) {
        const bool remap = want && cuzfp::decode_remap_ok(n, wpg, enc);
        if (want && !remap) continue;
        remapped += remap;
        // (the remap only where whole rounds of 8 workgroups of whole encoder workgroups)
        if (remap && (n % (8 * wpg) || wpg % enc || wpg <= enc)) bad++;
        const uint32_t groups = (n + wpg - 1) / wpg;
        std::vector<int> hit(n, 0);
        for (uint32_t gr = 0; gr < groups; gr++)
          for (uint32_t w = 0; w < wpg; w++) {
            const uint32_t v = cuzfp::decode_wave_of(gr, w, wpg, enc, remap);
            if (v < n)
              hit[v]++;
            else if (gr * wpg + w < n)
              bad++;  // a slot the launch needs maps past its end
            if (remap && (v / enc) % cuzfp::kXcds != gr % cuzfp::kXcds) bad++;
          }
        for (uint32_t v = 0; v < n; v++) bad += hit[v] != 1;
      }
  if (argc == 1 && !remapped) bad++;
  printf("%ld\n", bad);
  return bad != 0;
}
