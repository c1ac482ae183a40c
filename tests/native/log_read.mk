# tests/native/log_read.mk -- test drivers of the log record reader (run from this directory:
#   make -C tests/native -f log_read.mk <target>).
CXX ?= g++
LIBDIR := ../../nvlevelz_amd
CSRC := ../../nvlevelz_amd/csrc

# nvl::shims::DeviceLogReader through the in-tree engine (tests/test_log_read_dev.py)
liblog_read_harness.so: log_read_harness.cc ../../include/nvl_leveldb_shims.h ../../include/nvl_framing.h $(LIBDIR)/libnvl_crc32c.so
	$(CXX) -O2 -std=c++11 -fPIC -shared -Wall -Werror -I../../include -o $@ log_read_harness.cc \
	    -L$(LIBDIR) -lnvl_crc32c -Wl,-rpath,'$$ORIGIN/../../nvlevelz_amd'

# host-only ASan/UBSan build of the record rules and nvl_log_read (tests/test_log_read.py)
log_read_asan: log_read_asan.cc $(CSRC)/crc32c_framing.cpp $(CSRC)/crc32c_host.cpp $(CSRC)/crc32c_log_core.h \
    $(CSRC)/crc32c_log_read_core.h ../../include/nvl_framing.h
	$(CXX) -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
	    -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I../../include -I$(CSRC) -o $@ \
	    log_read_asan.cc $(CSRC)/crc32c_framing.cpp $(CSRC)/crc32c_host.cpp

clean:
	rm -f liblog_read_harness.so log_read_asan
