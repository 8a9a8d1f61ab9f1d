// A stand-alone driver of tests/cpp/retract_host_shim.hip for a host
// sanitizer run: build both with -Xarch_host -fsanitize=address,undefined and
// run the program on the CPU.  It walks the shim's entry points over designed
// runs (duplicates, two keys in one bucket, exact equality, one over, refused
// values) and returns non-zero when an answer is wrong.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" {
int rh_validate(const int64_t* rows, const float* vals, int64_t n, int64_t nrows, int frac_bits);
void rh_dec(const float* vals, int64_t n, int frac_bits, uint32_t* dec, uint8_t* ok);
void rh_combine(const uint32_t* bucket, const uint32_t* dec, int cnt, uint64_t* sum, uint8_t* leader);
int64_t rh_check_run(const uint32_t* bucket, const uint32_t* dec, int cnt, const uint32_t* counters, int w);
int rh_wave_run(void);
}

static int fails = 0;
#define EXPECT(c)                                              \
  do {                                                         \
    if (!(c)) {                                                \
      std::printf("%s:%d: %s\n", __FILE__, __LINE__, #c);      \
      ++fails;                                                 \
    }                                                          \
  } while (0)

int main() {
  {  // validation: rows, then values, at frac_bits 0 and 1
    const std::vector<int64_t> rows = {0, 3, 2};
    const std::vector<float> good = {1.0f, 0.0f, 2.5f};
    EXPECT(rh_validate(rows.data(), good.data(), 3, 4, 1) == 0);
    EXPECT(rh_validate(rows.data(), good.data(), 3, 4, 0) == 5);  // 2.5 is no integer
    EXPECT(rh_validate(rows.data(), good.data(), 3, 3, 1) == 1);  // row 3 of 3
    EXPECT(rh_validate(nullptr, nullptr, 3, 0, 0) == 0);
    const std::vector<float> bad = {-1.0f, 4294967296.0f, 2147483648.0f};
    std::vector<uint32_t> dec(3);
    std::vector<uint8_t> ok(3);
    rh_dec(bad.data(), 3, 0, dec.data(), ok.data());
    EXPECT(!ok[0] && !ok[1] && ok[2] && dec[2] == 2147483648u);
    rh_dec(bad.data(), 3, 1, dec.data(), ok.data());
    EXPECT(!ok[0] && !ok[1] && !ok[2]);
  }
  {  // one run of a wave's length: duplicates and shared buckets
    const int cnt = rh_wave_run(), w = 16;
    std::vector<uint32_t> bucket(cnt), dec(cnt), counters(w, 0);
    for (int t = 0; t < cnt; ++t) {
      bucket[t] = (uint32_t)((t * 7) % w);
      dec[t] = (uint32_t)(1 + t % 3);
      counters[bucket[t]] += dec[t];
    }
    std::vector<uint64_t> sum(cnt);
    std::vector<uint8_t> leader(cnt);
    rh_combine(bucket.data(), dec.data(), cnt, sum.data(), leader.data());
    int leaders = 0;
    for (int t = 0; t < cnt; ++t) {
      EXPECT(sum[t] == counters[bucket[t]]);
      leaders += leader[t];
    }
    EXPECT(leaders == w);
    EXPECT(rh_check_run(bucket.data(), dec.data(), cnt, counters.data(), w) == -1);  // exact equality passes
    counters[5] -= 1;
    counters[11] -= 1;
    EXPECT(rh_check_run(bucket.data(), dec.data(), cnt, counters.data(), w) == 5);  // one over: the smallest bucket
    EXPECT(rh_check_run(bucket.data(), dec.data(), 0, counters.data(), w) == -1);
  }
  std::printf(fails ? "retract_host_main: %d failures\n" : "retract_host_main: ok\n", fails);
  return fails ? 1 : 0;
}
