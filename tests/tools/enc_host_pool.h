// enc_host_pool.h -- TEST TOOL: what the two host models (mobi_encode_host.cpp, mobi_encode_inter_host.cpp) share: an encoder's constants
// built once, and the pool that deals pictures to threads.
#ifndef ENC_HOST_POOL_H
#define ENC_HOST_POOL_H
#include <atomic>
#include <stdint.h>
#include <thread>
#include <vector>

// the constants `build` makes (csrc: mobi_enc_build_const, mobi_encp_build_const), once per process and kept
template <class Const>
const Const *enc_host_const(void (*build)(Const *)) {
  static const Const *K = [build] {
    Const *k = new Const;
    build(k);
    return k;
  }();
  return K;
}

// n pictures dealt to `threads` workers: picture(i, forms) encodes picture i, counts the code forms it wrote into its thread's forms[4]
// and returns whether the bits written were the bits priced.  The threads' counts are added to forms (may be NULL).
// Returns 1 if some picture's were not, else 0.
template <class Picture>
int enc_host_pool(int n, int threads, uint32_t *forms, Picture picture) {
  std::atomic<int> next{0}, bad{0};
  std::vector<std::vector<uint32_t>> tforms(threads, std::vector<uint32_t>(4, 0));
  auto work = [&](int t) {
    for (int i; (i = next.fetch_add(1)) < n;)
      if (!picture(i, tforms[t].data())) bad++;
  };
  if (threads == 1) {
    work(0);
  } else {
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++) pool.emplace_back(work, t);
    for (auto &th : pool) th.join();
  }
  if (forms)
    for (int t = 0; t < threads; t++)
      for (int f = 0; f < 4; f++) forms[f] += tforms[t][f];
  return bad ? 1 : 0;
}
#endif
