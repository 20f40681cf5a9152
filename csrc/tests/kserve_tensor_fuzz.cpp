// Malformed-message driver for the tensor-model half of the KServe-v2 codec (csrc/runtime/kserve.cpp:
// kserve_parse_tensor_input, kserve_build_tensor_response, kserve_parse_tensor_response), built host-only under
// AddressSanitizer + UBSan by tests/test_native_tensor_serving.py.  Tensor requests reach the parser straight from
// the model server's public REST port and the front end then hands `n` items of `item_bytes` at `off` to the
// batcher without a copy, so whatever the parser accepts must lie inside the body.
//
//   kserve_tensor_fuzz [iterations]
//
// 1. fixed cases: the valid forms ([3,S,S], [N,3,S,S]) are located exactly; every malformed form of the issue
//    list (datatype, rank, channels, size mismatch, size past the body, header past the body, two inputs, unknown
//    input, N above max_batch_size, unknown output, JSON data, wrapping sizes, deep nesting) is rejected;
// 2. the builder's response parses back to the items it was given, and refuses items of the wrong size;
// 3. random byte flips, truncations, digit rewrites and bracket runs of valid requests and responses: any verdict,
//    an accepted one lies inside the body, no memory error.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "runtime/kserve.h"

namespace {

int failures = 0;

void expect(bool cond, const char* what) {
  if (!cond) {
    std::printf("FAIL: %s\n", what);
    ++failures;
  }
}

arena::KServeTensorModel model(int max_batch) {
  arena::KServeTensorModel m;
  m.name = "tiny";
  m.input = "images";
  m.output = "output0";
  m.max_batch_size = max_batch;
  m.in_dims = max_batch > 0 ? std::vector<int64_t>{3, 8, 8} : std::vector<int64_t>{1, 3, 8, 8};
  m.out_dims = max_batch > 0 ? std::vector<int64_t>{21} : std::vector<int64_t>{1, 21};
  return m;
}

bool parse_req(const std::string& body, int64_t ihcl, const arena::KServeTensorModel& m,
               arena::KServeTensorRequest* out = nullptr) {
  arena::KServeTensorRequest r;
  std::string err;
  const bool ok = arena::kserve_parse_tensor_input(body, ihcl, m, r, err);
  if (ok) {
    const uint64_t bytes = (uint64_t)r.n * (uint64_t)r.item_bytes;
    if (r.n < 1 || r.item_bytes != m.in_item_bytes() || r.off > body.size() || bytes > body.size() - r.off) {
      std::printf("FAIL: accepted items outside the body (off %zu n %lld item %lld size %zu)\n", r.off,
                  (long long)r.n, (long long)r.item_bytes, body.size());
      ++failures;
    }
  } else if (err.empty()) {
    std::printf("FAIL: rejection without a message\n");
    ++failures;
  }
  if (out) *out = r;
  return ok;
}

bool parse_resp(const std::string& body, int64_t ihcl, size_t* off = nullptr, size_t* len = nullptr,
                std::vector<int64_t>* shape = nullptr) {
  std::string name, err;
  std::vector<int64_t> sh;
  size_t o = 0, l = 0;
  const bool ok = arena::kserve_parse_tensor_response(body, ihcl, name, sh, o, l, err);
  if (ok && (o > body.size() || l > body.size() - o)) {
    std::printf("FAIL: accepted output outside the body\n");
    ++failures;
  }
  if (off) *off = o;
  if (len) *len = l;
  if (shape) *shape = sh;
  return ok;
}

// one input descriptor; `extra`: further members of the header object (", \"outputs\": ...")
std::string request(const std::string& name, const std::string& dtype, const std::string& shape, const std::string& size,
                    size_t payload, int64_t* ihcl, const std::string& extra = "", const std::string& more_inputs = "") {
  std::string h = "{\"id\":\"r1\",\"inputs\":[{\"name\":\"" + name + "\",\"shape\":" + shape + ",\"datatype\":\"" + dtype +
                  "\",\"parameters\":{\"binary_data_size\":" + size + "}}" + more_inputs + "]" + extra + "}";
  *ihcl = (int64_t)h.size();
  std::string p(payload, '\0');
  for (size_t i = 0; i < payload; ++i) p[i] = (char)(i * 7 + 1);
  return h + p;
}

}  // namespace

int main(int argc, char** argv) {
  const int iters = argc > 1 ? std::atoi(argv[1]) : 2000;
  const arena::KServeTensorModel m8 = model(8), m0 = model(0);
  const size_t item = 3 * 8 * 8 * 4;
  int64_t ihcl = -1;
  arena::KServeTensorRequest r;

  // ---- 1. fixed cases
  {
    std::string b = request("images", "FP32", "[1,3,8,8]", std::to_string(item), item, &ihcl);
    expect(parse_req(b, ihcl, m8, &r) && r.n == 1 && r.batch_dim && r.off == (size_t)ihcl && r.id == "r1",
           "[1,3,8,8] accepted and located");
    expect(parse_req(b, ihcl, m0, &r) && r.n == 1 && r.batch_dim, "[1,3,8,8] accepted without batching");
    b = request("images", "FP32", "[3,8,8]", std::to_string(item), item, &ihcl);
    expect(parse_req(b, ihcl, m8, &r) && r.n == 1 && !r.batch_dim, "[3,8,8] accepted, no batch dimension");
    b = request("images", "FP32", "[3,3,8,8]", std::to_string(3 * item), 3 * item, &ihcl);
    expect(parse_req(b, ihcl, m8, &r) && r.n == 3 && r.item_bytes == (int64_t)item, "[3,3,8,8] gives three items");
    expect(!parse_req(b, ihcl, m0), "N = 3 rejected when max_batch_size is 0");
    b = request("images", "FP32", "[1,3,8,8]", std::to_string(item), item, &ihcl,
                ",\"outputs\":[{\"name\":\"output0\",\"parameters\":{\"binary_data\":true}}]");
    expect(parse_req(b, ihcl, m8), "the model's own output may be named");
    b = request("images", "FP32", "[1,3,8,8]", std::to_string(item), item + 5, &ihcl);
    expect(parse_req(b, ihcl, m8), "trailing bytes after the tensor are tolerated");
  }
  {
    std::string b = request("images", "FP16", "[1,3,8,8]", std::to_string(item), item, &ihcl);
    expect(!parse_req(b, ihcl, m8), "wrong datatype rejected");
    b = request("images", "FP32", "[8,8]", std::to_string(item), item, &ihcl);
    expect(!parse_req(b, ihcl, m8), "rank 2 rejected");
    b = request("images", "FP32", "[1,1,3,8,8]", std::to_string(item), item, &ihcl);
    expect(!parse_req(b, ihcl, m8), "rank 5 rejected");
    b = request("images", "FP32", "[1,4,8,8]", std::to_string(4 * 8 * 8 * 4), 4 * 8 * 8 * 4, &ihcl);
    expect(!parse_req(b, ihcl, m8), "channel count 4 rejected");
    b = request("images", "FP32", "[1,3,8,8]", std::to_string(item - 4), item, &ihcl);
    expect(!parse_req(b, ihcl, m8), "binary_data_size != product(shape) * 4 rejected");
    b = request("images", "FP32", "[2,3,8,8]", std::to_string(2 * item), item, &ihcl);
    expect(!parse_req(b, ihcl, m8), "size running past the body rejected");
    b = request("images", "FP32", "[1,3,8,8]", std::to_string(item), item, &ihcl);
    expect(!parse_req(b, (int64_t)b.size() + 1, m8), "header length past the body rejected");
    expect(!parse_req(b, -1, m8), "missing Inference-Header-Content-Length rejected");
    b = request("images", "FP32", "[1,3,8,8]", std::to_string(item), 2 * item, &ihcl, "",
                ",{\"name\":\"more\",\"shape\":[1,3,8,8],\"datatype\":\"FP32\",\"parameters\":{\"binary_data_size\":" +
                    std::to_string(item) + "}}");
    expect(!parse_req(b, ihcl, m8), "two inputs rejected");
    b = request("input", "FP32", "[1,3,8,8]", std::to_string(item), item, &ihcl);
    expect(!parse_req(b, ihcl, m8), "unknown input name rejected");
    b = request("images", "FP32", "[9,3,8,8]", std::to_string(9 * item), 9 * item, &ihcl);
    expect(!parse_req(b, ihcl, m8), "N above max_batch_size rejected");
    b = request("images", "FP32", "[0,3,8,8]", "0", 0, &ihcl);
    expect(!parse_req(b, ihcl, m8), "N = 0 rejected");
    b = request("images", "FP32", "[-1,3,8,8]", std::to_string(item), item, &ihcl);
    expect(!parse_req(b, ihcl, m8), "negative N rejected");
    b = request("images", "FP32", "[1,3,8,8]", std::to_string(item), item, &ihcl,
                ",\"outputs\":[{\"name\":\"output1\"}]");
    expect(!parse_req(b, ihcl, m8), "unknown output name rejected");
    b = request("images", "FP32", "[4611686018427387904,3,8,8]", "0", 0, &ihcl);
    expect(!parse_req(b, ihcl, m8), "N that wraps the byte count rejected");
    b = request("images", "FP32", "[1,3,8,8]", "18446744073709551616", item, &ihcl);
    expect(!parse_req(b, ihcl, m8), "binary_data_size beyond 64 bits rejected");
    b = request("images", "FP32", "[1,3,8,8]", "-768", item, &ihcl);
    expect(!parse_req(b, ihcl, m8), "negative binary_data_size rejected");
    std::string js = "{\"inputs\":[{\"name\":\"images\",\"shape\":[1,3,8,8],\"datatype\":\"FP32\",\"data\":[0.5,1.5]}]}";
    expect(!parse_req(js, (int64_t)js.size(), m8), "JSON data input rejected (with the header length)");
    expect(!parse_req(js, -1, m8), "JSON data input rejected (without it)");
    const std::string deep = "{\"inputs\":" + std::string(1 << 20, '[');
    expect(!parse_req(deep, (int64_t)deep.size(), m8), "1 MB of '[' rejected");
  }

  // ---- 2. builder -> parser
  {
    std::vector<std::vector<uint8_t>> raw(3, std::vector<uint8_t>(84));
    for (size_t i = 0; i < raw.size(); ++i)
      for (size_t k = 0; k < 84; ++k) raw[i][k] = (uint8_t)(i * 100 + k);
    std::vector<const std::vector<uint8_t>*> items{&raw[0], &raw[1], &raw[2]};
    const std::string b = arena::kserve_build_tensor_response(m8, "id \"7\"", true, items, &ihcl);
    size_t off = 0, len = 0;
    std::vector<int64_t> shape;
    expect(parse_resp(b, ihcl, &off, &len, &shape) && len == 3 * 84 && shape == std::vector<int64_t>({3, 21}),
           "batched response parses back");
    expect(off + len == b.size() && std::memcmp(b.data() + off + 84, raw[1].data(), 84) == 0,
           "items follow the header in order");
    std::vector<const std::vector<uint8_t>*> one{&raw[2]};
    const std::string b1 = arena::kserve_build_tensor_response(m8, "", false, one, &ihcl);
    expect(parse_resp(b1, ihcl, &off, &len, &shape) && len == 84 && shape == std::vector<int64_t>({21}),
           "item-shaped response parses back");
    bool threw = false;
    try {
      std::vector<uint8_t> small(80);
      std::vector<const std::vector<uint8_t>*> bad{&small};
      arena::kserve_build_tensor_response(m8, "", true, bad, &ihcl);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    expect(threw, "an item of the wrong size is refused");
    threw = false;
    try {
      arena::kserve_build_tensor_response(m8, "", false, items, &ihcl);
    } catch (const std::invalid_argument&) {
      threw = true;
    }
    expect(threw, "three items without a batch dimension are refused");
    int64_t h2 = -1;
    const std::string huge = "{\"outputs\":[{\"name\":\"output0\",\"datatype\":\"FP32\",\"shape\":[4611686018427387904,4],"
                             "\"parameters\":{\"binary_data_size\":0}}]}";
    h2 = (int64_t)huge.size();
    expect(!parse_resp(huge, h2), "overflowing output shape rejected");
    expect(!arena::kserve_tensor_model_metadata(m8).empty() && !arena::kserve_tensor_model_metadata(m0).empty(),
           "metadata renders");
  }

  // ---- 3. random mutations
  std::mt19937 rng(4321);
  int64_t q_ihcl = -1, r_ihcl = -1;
  const std::string req = request("images", "FP32", "[2,3,8,8]", std::to_string(2 * item), 2 * item, &q_ihcl,
                                  ",\"outputs\":[{\"name\":\"output0\",\"parameters\":{\"binary_data\":true}}]");
  std::vector<uint8_t> out_item(84, 3);
  std::vector<const std::vector<uint8_t>*> two{&out_item, &out_item};
  const std::string resp = arena::kserve_build_tensor_response(m8, "id-1", true, two, &r_ihcl);
  for (int it = 0; it < iters; ++it) {
    const bool is_req = (it & 1) == 0;
    std::string m = is_req ? req : resp;
    int64_t h = is_req ? q_ihcl : r_ihcl;
    const int edits = 1 + (int)(rng() % 4);
    for (int e = 0; e < edits; ++e) {
      const int kind = (int)(rng() % 5);
      if (m.empty()) break;
      const size_t pos = rng() % m.size();
      if (kind == 0) {
        m[pos] = (char)(rng() & 0xff);
      } else if (kind == 1) {
        m.resize(pos);
      } else if (kind == 2 && h > 0 && pos < (size_t)h) {
        if (m[pos] >= '0' && m[pos] <= '9') m.insert(pos, std::string(1 + rng() % 18, (char)('0' + rng() % 10)));
      } else if (kind == 3 && h > 0 && pos < (size_t)h) {
        m.insert(pos, std::string(1 + rng() % 64, (rng() & 1) ? '[' : '{'));
      } else {
        h = (int64_t)(rng() % (m.size() + 8)) - 4;
      }
    }
    if (is_req) parse_req(m, h, (it & 2) ? m8 : m0);
    else parse_resp(m, h);
  }
  if (failures) {
    std::printf("kserve_tensor_fuzz: %d failures\n", failures);
    return 1;
  }
  std::printf("kserve_tensor_fuzz: ok (%d mutations)\n", iters);
  return 0;
}
