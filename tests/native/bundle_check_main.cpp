// Stand-alone driver of the host-only bundle reader (stable-renderer_amd/csrc/bundle_file.h): no HIP, no GPU.
//   bundle_check [--limit BYTES] PATH...   one line per file (a directory = its files, sorted by name):
//        <path> TAB <return code> TAB <message, "ok" when accepted> TAB <plan:op:field:tensor:offset:bytes of every validated pointer>
//   bundle_check --fields                  one line per op kind 1..15: <kind> TAB <offset:name,...> (the C++ pointer-field table)
//   bundle_check --sizes                   sizeof(sr_op), and the groupnorm scratch formula on a few (B, HW)
// tests/test_bundle_file.py builds it (with the address and undefined-behaviour sanitizers where no GPU is visible) and runs it as a
// child process.
#include "../../stable-renderer_amd/csrc/bundle_file.h"
#include <algorithm>
#include <filesystem>
#include <stdlib.h>

static void check_file(const std::string& path, uint64_t limit) {
  sr_bundle::Bundle b;
  std::string err;
  const int rc = sr_bundle::read(path.c_str(), limit, &b, &err);
  for (char& c : err) if (c == '\t' || c == '\n') c = ' ';
  printf("%s\t%d\t%s\t", path.c_str(), rc, rc == SR_OK ? "ok" : err.c_str());
  if (rc == SR_OK)
    for (size_t i = 0; i < b.extents.size(); ++i) {
      const sr_bundle::Extent& e = b.extents[i];
      printf("%s%u:%u:%s:%u:%llu:%llu", i ? " " : "", e.plan, e.op, e.field, e.tensor, (unsigned long long)e.offset, (unsigned long long)e.bytes);
    }
  printf("\n");
}

int main(int argc, char** argv) {
  uint64_t limit = 0;
  std::vector<std::string> paths;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--fields") {
      for (int kind = 1; kind <= 15; ++kind) {
        printf("%d\t", kind);
        const std::vector<sr_bundle::Field> pf = sr_bundle::pointer_fields(kind);
        for (size_t k = 0; k < pf.size(); ++k) printf("%s%zu:%s", k ? "," : "", pf[k].offset, pf[k].name);
        printf("\n");
      }
      return 0;
    }
    if (a == "--sizes") {
      printf("sizeof_op\t%zu\n", sizeof(sr_op));
      for (int i2 = i + 1; i2 + 1 < argc; i2 += 2)
        printf("gn\t%s\t%s\t%llu\n", argv[i2], argv[i2 + 1], (unsigned long long)sr_bundle::gn_scratch_floats(atoll(argv[i2]), atoll(argv[i2 + 1])));
      return 0;
    }
    if (a == "--limit" && i + 1 < argc) { limit = strtoull(argv[++i], nullptr, 10); continue; }
    paths.push_back(a);
  }
  if (paths.empty()) { fprintf(stderr, "usage: bundle_check [--limit BYTES] PATH... | --fields | --sizes [B HW]...\n"); return 2; }
  for (const std::string& p : paths) {
    std::error_code ec;
    if (std::filesystem::is_directory(p, ec)) {
      std::vector<std::string> files;
      for (const auto& e : std::filesystem::directory_iterator(p, ec))
        if (e.is_regular_file()) files.push_back(e.path().string());
      std::sort(files.begin(), files.end());
      for (const std::string& f : files) check_file(f, limit);
    } else
      check_file(p, limit);
  }
  return 0;
}
