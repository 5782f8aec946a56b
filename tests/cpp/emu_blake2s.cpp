// Host emulation of the functions behind jj_blake2s and jj_group_hash's hash (jubjub_amd/csrc/jj_blake2s.h compiled with -DJJ_HOST_EMU): the
// host's midstate over the whole blocks of a prefix (Blake2s::midstate_blocks, Blake2s::midstate) and what one lane of k_blake2s does with it
// (Blake2s::finish over the prefix's tail and the lane's message), as a stand-alone program.  Test infrastructure only
// (tests/test_emu_blake2s.py); nothing in jubjub_amd/ links or loads it.
//
// argv[1]: a file that tests/test_emu_blake2s.py writes,
//   8 bytes of personalisation | PREFIX_POOL bytes | MSG_POOL bytes | one 32-byte digest of hashlib per case,
// the cases in the order  prefix_len 0..200, msg_len 0..140, skew 0..3:  prefix = the pool's first prefix_len bytes, message = msg_len bytes of
// the message pool from (3 prefix_len + 5 msg_len + 7 skew) mod 128, personalisation absent (eight zero bytes) where prefix_len + msg_len is a
// multiple of 5.  stdout: "<cases> cases, <mismatches> mismatches"; exit status 1 on a mismatch.
// The prefix is copied into a fresh allocation of exactly its length and the message to byte `skew` of a fresh allocation that ends with the
// dword of its last byte, so a build with -fsanitize=address reports a read past the prefix and a load of a dword that holds no byte of the
// message; an absent prefix and an empty message are handed over as null pointers.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#define JJ_HOST_EMU 1
#include "../../jubjub_amd/csrc/jj_blake2s.h"

using namespace jj;

extern "C" void jj_emu_overflow(const char*) {}

static const size_t PREFIX_POOL = 256, MSG_POOL = 512, PREFIX_MAX = 200, MSG_MAX = 140;

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: emu_blake2s FILE\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  const size_t cases = (PREFIX_MAX + 1) * (MSG_MAX + 1) * 4;
  std::vector<uint8_t> data(8 + PREFIX_POOL + MSG_POOL + 32 * cases);
  if (fread(data.data(), 1, data.size(), f) != data.size() || fgetc(f) != EOF) { fprintf(stderr, "bad file\n"); return 2; }
  fclose(f);
  const uint8_t* personal = data.data();
  const uint8_t* ppool = personal + 8;
  const uint8_t* mpool = ppool + PREFIX_POOL;
  const uint8_t* want = mpool + MSG_POOL;
  size_t bad = 0, k = 0;
  for (size_t pl = 0; pl <= PREFIX_MAX; pl++)
    for (size_t ml = 0; ml <= MSG_MAX; ml++)
      for (size_t skew = 0; skew < 4; skew++, k++) {
        uint8_t* prefix = nullptr;
        if (pl) { prefix = (uint8_t*)malloc(pl); memcpy(prefix, ppool, pl); }
        uint8_t* buf = nullptr;
        if (ml) {
          buf = (uint8_t*)malloc((skew + ml + 3) & ~(size_t)3);          // malloc's alignment stands for the 16 bytes asked of a device pointer
          memset(buf, 0xA5, skew);
          memcpy(buf + skew, mpool + (3 * pl + 5 * ml + 7 * skew) % 128, ml);
        }
        const size_t B = Blake2s::midstate_blocks(pl, ml);
        u32 h[8], tail[16], out[8];
        Blake2s::midstate(h, tail, (pl + ml) % 5 == 0 ? nullptr : personal, prefix, pl, B);
        Blake2s::finish(out, h, tail, (u32)(64 * B), (u32)(pl - 64 * B), buf, (u32)skew, (u32)ml);
        free(prefix); free(buf);
        uint8_t got[32];
        for (int j = 0; j < 8; j++) { got[4 * j] = (uint8_t)out[j]; got[4 * j + 1] = (uint8_t)(out[j] >> 8); got[4 * j + 2] = (uint8_t)(out[j] >> 16); got[4 * j + 3] = (uint8_t)(out[j] >> 24); }
        if (memcmp(got, want + 32 * k, 32) != 0) {
          if (bad++ < 8) fprintf(stderr, "mismatch: prefix_len %zu msg_len %zu skew %zu (B = %zu)\n", pl, ml, skew, B);
        }
      }
  printf("%zu cases, %zu mismatches\n", k, bad);
  return bad ? 1 : 0;
}
