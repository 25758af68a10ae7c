# Build of the MI355X (gfx950) SIFT path.  Outputs stay in-tree so they
# travel to the GPU box with the snapshot (they are git-ignored).
# OBJDIR, LIB and EXTRA (more compile flags) are for tools/build_variant.sh.
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
PKG     := sift-scale-space-extrema-detection_amd
CSRC    := $(PKG)/csrc
HIPSRC  := $(wildcard $(CSRC)/*.hip)
HDRS    := $(wildcard $(CSRC)/*.h) include/sift_hip.h
HIPFLAGS ?= --offload-arch=$(ARCH) -O3 -fPIC -std=c++17 -Wall -Wno-unused-result
OBJDIR  ?= $(PKG)/build
LIB     ?= $(PKG)/libsift_hip.so
OBJS    := $(patsubst $(CSRC)/%.hip,$(OBJDIR)/%.o,$(HIPSRC))

all: lib oracle
lib: $(LIB)

$(OBJDIR)/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) $(EXTRA) -c -o $@ $<

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS)

oracle:
	$(MAKE) -C oracle

clean:
	rm -rf $(OBJDIR) $(LIB)
	$(MAKE) -C oracle clean

.PHONY: all lib oracle clean
