// scalar_sim.cpp -- scalar_dev.h (arithmetic mod the group order of secp256k1) on the host, as a
// stand-alone program: tests/test_sig.py builds it with the sanitizers on and compares its output with
// Python integers.
//
//   scalar_sim OPERANDS
// OPERANDS holds one operation per line, numbers as 64 hex digits:
//   mul A B   -> A B mod n
//   inv A     -> A^-1 mod n
//   add A B   -> A + B mod n (A, B < n)
//   rec U     -> U made odd and recoded (0 < U < n): the flip flag and the 64 digits, least significant first
// One line of output per line of input.
#include <cstdio>
#include <cstring>

#include "scalar_dev.h"

static bool parse(const char* h, sn::sc& a) {
  if (std::strlen(h) != 64) return false;
  for (int i = 0; i < 8; ++i) {
    unsigned v = 0;
    if (std::sscanf(h + 8 * i, "%8x", &v) != 1) return false;
    a.d[7 - i] = v;
  }
  return true;
}

static void print(const sn::sc& a) {
  for (int i = 7; i >= 0; --i) std::printf("%08x", a.d[i]);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char op[8], x[80], y[80];
  char line[256];
  while (std::fgets(line, sizeof line, f)) {
    const int got = std::sscanf(line, "%7s %79s %79s", op, x, y);
    sn::sc a, b, r;
    if (got < 2 || !parse(x, a)) return 3;
    if (!std::strcmp(op, "mul")) {
      if (got != 3 || !parse(y, b)) return 3;
      sn::mul(r, a, b);
      print(r);
    } else if (!std::strcmp(op, "add")) {
      if (got != 3 || !parse(y, b)) return 3;
      sn::add(r, a, b);
      print(r);
    } else if (!std::strcmp(op, "inv")) {
      sn::inv(r, a);
      print(r);
    } else if (!std::strcmp(op, "rec")) {
      const bool flip = sn::make_odd(r, a);
      std::printf("%d", flip ? 1 : 0);
      for (int i = 0; i < 64; ++i) std::printf(" %d", sn::recode_digit(r, i));
      std::printf("\n");
    } else {
      return 3;
    }
  }
  std::fclose(f);
  return 0;
}
