import os, sys
sys.path.insert(0, os.getcwd())
os.environ["RXR_SHADER_JIT"] = "1"; os.environ["RXR_JIT_CACHE"] = "0"
import ctypes as C
import rusterix_amd
from rusterix_amd import scenes
prod = rusterix_amd.load()
cfg = scenes.box_grid_scene(prod, n=96, width=1920, height=1080, shader=True)
scenes.render(cfg)
rxr = rusterix_amd.rxr_abi()
print(rxr.rxr_debug_jit_info(prod.lib.rxh_context()).decode())
