// Host build of the checkpoint image's validation (mahout_amd/csrc/cms_checkpoint.cpp)
// for tests/test_checkpoint_host.py: each call returns NULL for a valid part,
// else the reason it is refused.
#include "../../mahout_amd/csrc/cms_checkpoint.h"

using namespace cms::ckpt;

extern "C" {

int host_header_bytes() { return (int)sizeof(Header); }
int host_dir_entry_bytes() { return (int)sizeof(DirEntry); }

void host_layout_sections(void* hd) { layout_sections(static_cast<Header*>(hd)); }

const char* host_check_header(const void* hd, uint64_t avail) { return check_header(*static_cast<const Header*>(hd), avail); }

const char* host_check_owner_ids(const int64_t* ids, int64_t n) { return check_owner_ids(ids, n); }

const char* host_check_directory(const void* hd, const void* dir, int64_t n) {
  return check_directory(*static_cast<const Header*>(hd), static_cast<const DirEntry*>(dir), n);
}

}  // extern "C"
