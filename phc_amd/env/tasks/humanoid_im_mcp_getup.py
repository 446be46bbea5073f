"""HumanoidImMCPGetup = primitive composer + fall recovery (reference: phc/env/tasks/humanoid_im_mcp_getup.py), the task of
env_im_getup_mcp.yaml (config 3's last stage)."""
from .humanoid_im_getup import HumanoidImGetup
from .humanoid_im_mcp import MCPMixin


class HumanoidImMCPGetup(MCPMixin, HumanoidImGetup):
    pass
