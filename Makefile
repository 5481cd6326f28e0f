# Build the gfx950 HIP library in-tree (the .so travels to the GPU box with the snapshot).
HIPCC ?= /opt/rocm/bin/hipcc
ARCH  ?= gfx950
SRC   := innfer_amd/csrc/conv3x3.hip innfer_amd/csrc/hr_chain.hip innfer_amd/csrc/conv_first.hip innfer_amd/csrc/conv_first_unshuffle.hip innfer_amd/csrc/shuffle_add.hip innfer_amd/csrc/plk_conv.hip innfer_amd/csrc/group_norm.hip innfer_amd/csrc/win_attn.hip innfer_amd/csrc/win_attn16.hip innfer_amd/csrc/win_attn16_wide.hip innfer_amd/csrc/chan_attn.hip innfer_amd/csrc/win_attn_rect.hip innfer_amd/csrc/chan_self_attn.hip innfer_amd/csrc/dwconv.hip innfer_amd/csrc/aim_mix.hip innfer_amd/csrc/dat_launches.hip innfer_amd/csrc/layer_norm.hip innfer_amd/csrc/tiles.hip innfer_amd/csrc/tiles_u8.hip innfer_amd/csrc/tiles_u8_multi.hip innfer_amd/csrc/tiles_tta.hip innfer_amd/csrc/tiles_stitch.hip innfer_amd/csrc/net.hip innfer_amd/csrc/unet.hip innfer_amd/csrc/pan.hip innfer_amd/csrc/pan_scpa.hip innfer_amd/csrc/pan_scpa_split.hip innfer_amd/csrc/f32ops.hip innfer_amd/csrc/colorfix.hip innfer_amd/csrc/resample.hip innfer_amd/csrc/ppon.hip innfer_amd/csrc/resnet.hip innfer_amd/csrc/wbcunet.hip innfer_amd/csrc/comm.hip
OBJ   := $(SRC:.hip=.o)
LIB   := innfer_amd/lib/libinnfer_amd.so
FLAGS := --offload-arch=$(ARCH) -O3 -fPIC -std=c++17 -Wall -Wno-unused-function

all: $(LIB)

innfer_amd/csrc/tiles.o innfer_amd/csrc/tiles_u8.o innfer_amd/csrc/tiles_u8_multi.o innfer_amd/csrc/tiles_tta.o innfer_amd/csrc/tiles_stitch.o innfer_amd/csrc/colorfix.o innfer_amd/csrc/resample.o: FLAGS += -ffp-contract=off

%.o: %.hip $(wildcard innfer_amd/csrc/*.h) $(wildcard innfer_amd/csrc/*.inc) include/innfer_amd.h
	$(HIPCC) $(FLAGS) -c $< -o $@

$(LIB): $(OBJ)
	@mkdir -p innfer_amd/lib
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJ) -ldl

# diagnostic library with in-kernel s_memtime stamps (never shipped, never benchmarked)
stamps:
	@mkdir -p build/stamps
	$(HIPCC) $(FLAGS) -DINNFER_STAMPS -DINNFER_ABLATE -shared -o innfer_amd/lib/libinnfer_amd_stamps.so $(SRC)

# diagnostic library whose conv kernel can skip its stores / DMA / MFMA phase (INNFER_ABL bits; never shipped)
ablate:
	$(HIPCC) $(FLAGS) -DINNFER_ABLATE -shared -o innfer_amd/lib/libinnfer_amd_ablate.so $(SRC)

clean:
	rm -f $(OBJ) $(LIB)

.PHONY: all clean stamps ablate
