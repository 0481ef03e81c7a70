// Stand-alone host program over the Ed25519 math the kernels of zkt_ed25519.hip run (sha512.h, fe25519.h, ed25519.h): keys, signatures and verifications at
// the block-edge message lengths and every byte alignment, with every buffer an exact-size heap block so that a read or write past one is caught.
// Built with the address and undefined-behaviour sanitizers by tests/test_ed25519_hostcheck.py and run as a program of its own; prints "ed25519 ok".
#include <vector>
#include <cstdio>
#include <cstring>
#include "ed25519.h"
using namespace zkt;
int main() {
  std::vector<uint32_t> tab((size_t)ED_COMB_ENTRIES * ED_PRE_WORDS);
  for (int e = 0; e < ED_COMB_ENTRIES; ++e) ed25519_comb_entry(e, tab.data() + (size_t)e * ED_PRE_WORDS);
  int bad = 0;
  const int lens[] = {0, 1, 47, 48, 49, 63, 64, 65, 111, 112, 113, 127, 128, 129, 1023};
  for (int li = 0; li < 15; ++li) for (int a = 0; a < 8; ++a) {
    const int len = lens[li];
    std::vector<uint8_t> m(len + a); for (int i = 0; i < len + a; ++i) m[i] = (uint8_t)(i * 7 + li);      // exact-size heap block: a read past the message is caught
    std::vector<uint8_t> prv(32 + a), pub(32 + a), sig(64 + a);
    for (int i = 0; i < 32; ++i) prv[a + i] = (uint8_t)(i + li + a);
    ed25519_public_key_one(prv.data() + a, tab.data(), pub.data() + a);
    ed25519_sign_one(m.data() + a, len, prv.data() + a, tab.data(), sig.data() + a);
    uint32_t wt[ED_TAB * ED_CW];
    if (!ed25519_verify_one<1>(m.data() + a, len, sig.data() + a, pub.data() + a, tab.data(), wt)) ++bad;
    sig[a + 5] ^= 1;
    if (ed25519_verify_one<1>(m.data() + a, len, sig.data() + a, pub.data() + a, tab.data(), wt)) ++bad;
    uint64_t h[8]; sha512_words<0>(nullptr, m.data() + a, len, h);
  }
  printf(bad ? "ed25519 bad=%d\n" : "ed25519 ok\n", bad);
  return bad;
}
